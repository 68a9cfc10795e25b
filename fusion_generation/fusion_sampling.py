#!/usr/bin/env python3
"""Drop-in for the reference's `python fusion_generation/fusion_sampling.py ...` (Custom-Diffusion weights).

Accepts the reference's argv unchanged (flags of fusion_sampling.py:534-585; `+`-separated lists, background
concept last) and runs the same Tweedie-mix loop on the MI355X-native sampler.  What the reference does around
the loop through the HF hub (checkpoint download) takes local paths here:

  --sd_path              local SDXL checkpoint in diffusers layout (unet/, text_encoder/, text_encoder_2/, tokenizer/,
                         tokenizer_2/, optionally vae/): prompts are tokenised and encoded natively (tweediemix_amd/text.py,
                         modifier tokens of --personal_checkpoint injected), the UNet comes from unet/
  --vae_path             VAE folder or weights file (the reference uses madebyollin/sdxl-vae-fp16-fix); with a VAE the
                         final image is written as {output_path_all}/{prompt_orig}_{seed}.png like the reference
  --unet_path            diffusers-format SDXL UNet weights (.safetensors / torch state dict); the concept
                         checkpoints of --personal_checkpoint (delta-*.bin, key 'unet') load unchanged
  --text_embeds_path     precomputed embeddings instead of the text towers: torch file
                         {'text_embeds': (E[K+2,77,2048], P[K+2,1280]), 'text_embeds_single': (E[K,77,2048], P[K,1280])}
  --mask_paths           '+'-separated 8-bit masks for the foreground concepts (what run_expand.py would write
                         as '<concept>.jpg'); --random_masks draws seeded rectangles instead
  --synthetic            random-init weights / embeddings of the SDXL shapes (no checkpoints exist offline)
  --mask_source attention  masks from the cross-attention maps of the look-ahead instead of the segmentation side-car: no VAE,
                         no second process.  Token positions of every --seg_concepts phrase in --prompt_orig (checkpoint
                         tokenizer), or --mask_token_ids '4+7' ('+' between concepts, ',' between positions of one) where
                         there is no tokenizer; --attn_mask_threshold, --save_attention_maps (raw maps as .npy).
                         --attn_mask_propagate N (0..3, default 0) pushes the maps N times through the self-attention of the last
                         look-ahead call before they are thresholded: a response on part of an object spreads over the object.
                         --attn_mask_shape free keeps the object's own outline instead of its bounding rectangle: the largest connected
                         component of the thresholded score, holes filled (--attn_mask_keep_holes: not), every pixel that several concepts
                         claim given to the highest score, so the masks of any number of concepts are disjoint.  Each rank
                         writes the masks it used as '<seg_concept>.jpg' into its side-car directory.  --mask_paths and
                         --random_masks still win over it
  --long_prompts         prompts past CLIP's 77 tokens: every prompt row (negative, scene, per-concept) is cut into chunks of 75 tokens at
                         word boundaries, each chunk encoded on its own, the hidden states concatenated: 154 or 231 cross-attention
                         keys (at most 3 chunks = 225 tokens; more is an error, nothing is dropped).  A run whose prompts all fit one
                         chunk is bit for bit the run without the flag.  --mask_token_ids then takes positions 77 * chunk + offset,
                         --text_embeds_path embeddings of [*, 77 c, 2048], and --synthetic draws --synthetic_chunks c x 77 keys
  --keep_latents FILE    hold an earlier result while the loop samples only the --reroll regions anew: FILE is the '.latent.pt' a run
                         wrote ([1,4,h,w] of this resolution).  Needs --mask_paths (the regions must be known before the first step) and
                         --reroll; everything outside the regions comes back bit for bit in the final latent.  With --num_seeds N every
                         seed re-rolls the same regions of the same image, sharing every UNet launch
  --keep_image FILE      the same with an RGB image of exactly resolution_w x resolution_h: kept is the VAE encoder's mean times the scaling
                         factor (nothing is drawn).  Excludes --keep_latents
  --reroll LIST          the regions sampled anew: '+'-separated --seg_concepts phrases or 0-based indices into them ('a dog', '1', '0+a dog')
  --mask_feather PX      SOFT REGION MASKS: the blend weights of every mask source (side-car, --mask_source attention, --mask_paths, the
                         rectangles) come from the distance to each region's border.  PX image pixels (the kernel gets PX / 8 latent
                         pixels) is the full width of the ramp around the border; --mask_dilate PX grows every region first (negative:
                         shrinks it); --mask_normalize divides the foreground weights by their sum where regions overlap, so that the
                         weights are a partition of unity (the reference does not normalise: there the overlap doubles at every fusion
                         step).  On a canvas the weights are built on the canvas grid.  All defaults (and --mask_feather up to 8 alone) are
                         today's run bit for bit.  With one of the flags each rank writes the foreground weights it used as
                         '<seg_concept>_soft.png' (8-bit) into its side-car directory
  --reroll_feather PX / --reroll_dilate PX  the same for the keep region: they act on the union of the --reroll regions, the kept
                         weight is 1 - (that union, dilated and feathered).  Where the kept weight is 1 the image still comes back bit for
                         bit; inside the ramp (0 < weight < 1) it is a blend of the kept image and the new sample and does not
  --canvas_h / --canvas_w  a WIDE CANVAS in pixels (0: the window, i.e. none): the picture is sampled as overlapping windows of
                         resolution_h x resolution_w that share every UNet launch like co-batched seeds and are reconciled after every
                         step; --window_overlap is their minimum overlap in pixels (default: half the smaller window side).  At most 8
                         windows; masks (--mask_paths, --random_masks, the synthetic rectangles) are built on the canvas grid, the
                         '.latent.pt' and '.png' are canvas-sized.  Not with --keep_*, --mask_source attention or --streams 2
  --solver dpmpp2m       every trajectory step behind the first timestep is a DPM-Solver++(2M) step on the blended Tweedie estimate (second
                         order from the second step of a phase on; no extra UNet call); --timestep_spacing logsnr places
                         the n_timesteps uniformly in log-SNR between the 'leading' grid's first timestep and t = 1, the fusion window
                         keeping its noise range.  Meant for a small --n_timesteps (10 .. 20); the defaults (ddim, leading) are today's
                         run bit for bit.  --solver dpmpp2m does not combine with --keep_latents / --keep_image
  --guidance_rescale PHI std-matched CFG (arXiv:2305.08891 section 3.4, diffusers' guidance_rescale): in every step each concept row's guided
                         prediction is scaled by PHI * sd(conditional) / sd(guided) + (1 - PHI), per UNet row (on a canvas: per window), against
                         the over-exposed look of a high --guidance_scale.  0 (default): off, today's run bit for bit; 0.7 is the paper's
                         value.  Two small launches per step, no UNet call.  Does not combine with --keep_latents / --keep_image
  --eta E                stochastic sampling, E in [0, 1]: every step that advances the trajectory adds noise, a pure function of (the
                         trajectory's seed, the schedule step, the canvas coordinate) computed inside the fused step kernel -- the same bits
                         alone, co-batched, on another GPU, eagerly or from a graph, and identical where canvas windows overlap.  --solver ddim:
                         the DDIM paper's eta; --solver dpmpp2m: SDE-DPM-Solver++(2M) in k-diffusion's eta form; the two definitions coincide at
                         0 and 1 and differ in between.  0 (default): today's run bit for bit.  Does not combine with
                         --keep_latents / --keep_image
  --guidance_interval T_HI,T_LO   guidance in a limited interval (arXiv:2404.07724): two integer timesteps, 1000 >= T_HI >= T_LO >= 0; a timestep
                         t is guided iff T_LO <= t <= T_HI.  Outside it the trajectory step (behind the first timestep) uses the conditional
                         prediction alone and its UNet call runs WITHOUT the unconditional row: K rows for a fusion call, one for a plain call
                         (DESIGN.md 7q).  Timestep values, not schedule indices: the interval keeps its noise range under --timestep_spacing
                         logsnr.  Without the flag, or with an interval that holds every timestep of the schedule: today's run bit for bit.
                         Does not combine with --keep_latents / --keep_image
  --apg                  adaptive projected guidance (Sadat, Hilliges and Weber, arXiv:2410.02416): every guided step forms its guidance on the
                         rows' Tweedie estimates, splits the update D_c - D_u into the part parallel to the conditional estimate D_c (the one
                         that inflates contrast and saturation at a high --guidance_scale) and the rest, keeps the rest, scales the parallel
                         part by --apg_eta ETA (default 0; 1 is CFG) and clips the update's norm over one UNet row at --apg_norm R (default 0:
                         no clip).  Statistics are per UNet row (on a canvas: per window); two small launches per guided step, no UNet call
                         (DESIGN.md 7s).  No momentum.  Without the flag: today's run bit for bit; --apg_eta / --apg_norm without it are
                         refused.  Does not combine with --guidance_rescale, --keep_latents / --keep_image
  --num_seeds N          N trajectories, seeds seed..seed+N-1 (trajectory i is exactly what `--seed seed+i` alone produces: its
                         x_T comes from its own generator), co-batched --seeds_per_batch at a time
  --gpus G               shard those seeds round-robin over G GPUs of this node: the script starts one process per GPU itself
                         (or runs under torch.distributed.run), every rank samples its seeds, the final latents are gathered
                         over RCCL and rank 0 writes the files (BASELINE config 4; the reference is single-GPU, sample_catdog.sh:3)

Output: {output_path_all}/{prompt_orig}_{seed}.latent.pt, plus the .png when VAE weights are given (a prompt of more than 200 bytes:
its first 160 characters and 8 hex digits of its SHA-1, see output_stem).
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LORA = False


def build_parser():
    p = argparse.ArgumentParser()
    # --- the reference's flags, same names / defaults (fusion_sampling.py:534-585); output_path / output_path_all have no
    # default there (None crashes at os.makedirs), here they fall back to ./results{,_all}
    p.add_argument('--seed', type=int, default=182)
    p.add_argument('--device', type=str, default='cuda:0')
    p.add_argument('--output_path', type=str, default='results')
    p.add_argument('--output_path_all', type=str, default='results_all')
    p.add_argument('--negative_prompt', type=str, default='blurry, ugly, black, low res, unrealistic, blurry face')
    p.add_argument('--sd_version', type=str, default='2.1', choices=['1.4', '1.5', '2.0', '2.1', 'xl'])
    p.add_argument('--t_cond', type=float, default=0.4)
    p.add_argument('--guidance_scale', type=float, default=9.0)
    p.add_argument('--n_timesteps', type=int, default=50)
    p.add_argument('--prompt', type=str, default='')
    p.add_argument('--prompt_orig', type=str, default='')
    p.add_argument('--seg_concepts', type=str, default='')
    p.add_argument('--personal_checkpoint', type=str, default='')
    p.add_argument('--concepts', type=str, default='')
    p.add_argument('--modifier_token', type=str, default='')
    p.add_argument('--resampling_steps', type=int, default=10)
    p.add_argument('--jumping_steps', type=int, default=5)
    p.add_argument('--seg_gpu', type=int, default=1)
    p.add_argument('--crops_coords_top_left_h', type=int, default=0)
    p.add_argument('--crops_coords_top_left_w', type=int, default=0)
    p.add_argument('--resolution_h', type=int, default=1024)
    p.add_argument('--resolution_w', type=int, default=1024)
    if LORA:
        p.add_argument('--t_stop', type=float, default=0.9)          # fusion_sampling_lora.py:547
    # --- additive flags
    p.add_argument('--synthetic', action='store_true')
    p.add_argument('--sd_path', type=str, default='')
    p.add_argument('--vae_path', type=str, default='')
    p.add_argument('--unet_path', type=str, default='')
    p.add_argument('--text_embeds_path', type=str, default='')
    p.add_argument('--mask_paths', type=str, default='')
    p.add_argument('--random_masks', action='store_true')
    p.add_argument('--mask_source', type=str, default='sidecar', choices=['sidecar', 'attention'],
                   help='attention: blend masks from the cross-attention maps of the look-ahead (no side-car, no VAE)')
    p.add_argument('--attn_mask_threshold', type=float, default=0.5)
    p.add_argument('--mask_token_ids', type=str, default='',
                   help="token positions per foreground concept, '+' between concepts, ',' within one (e.g. '4+7')")
    p.add_argument('--save_attention_maps', action='store_true')
    p.add_argument('--attn_mask_propagate', type=int, default=0,
                   help='--mask_source attention: rounds (0..3) of pushing the token maps through the self-attention before thresholding')
    p.add_argument('--attn_mask_shape', type=str, default='rect', choices=['rect', 'free'],
                   help="--mask_source attention: 'rect' the bounding rectangle of every mask (the side-car's rule), 'free' the object's own outline, "
                        "holes filled, overlaps resolved towards the highest score")
    p.add_argument('--attn_mask_keep_holes', action='store_true', help='--attn_mask_shape free: do not fill the holes of an outline')
    p.add_argument('--long_prompts', action='store_true',
                   help='chunked prompts: 75-token chunks encoded one by one and concatenated (77 c cross-attention keys, c <= 3)')
    p.add_argument('--synthetic_chunks', type=int, default=1, help='--synthetic with --long_prompts: embeddings of 77 * c keys (c in 1..3)')
    p.add_argument('--keep_latents', type=str, default='', help="'.latent.pt' of an earlier run: kept outside the --reroll regions")
    p.add_argument('--keep_image', type=str, default='', help='RGB image of resolution_w x resolution_h: its VAE encoding is kept outside the --reroll regions')
    p.add_argument('--reroll', type=str, default='', help="regions sampled anew: '+'-separated --seg_concepts phrases or 0-based indices into them")
    p.add_argument('--mask_feather', type=float, default=0.0, help='soft masks: full width in image pixels of the ramp around every region border (>= 0; up to 8 alone: the hard masks)')
    p.add_argument('--mask_dilate', type=float, default=0.0, help='soft masks: grow every region by this many image pixels before the ramp (negative: shrink)')
    p.add_argument('--mask_normalize', action='store_true', help='soft masks: where regions overlap, divide the foreground weights by their sum (weights sum to 1 everywhere)')
    p.add_argument('--reroll_feather', type=float, default=0.0,
                   help='keep region: ramp width in image pixels around the union of the --reroll regions.  Where the kept weight is 1 the kept image still '
                        'returns bit for bit; where 0 < weight < 1 it is blended with the new sample and does not')
    p.add_argument('--reroll_dilate', type=float, default=0.0, help='keep region: grow the union of the --reroll regions by this many image pixels (negative: shrink)')
    p.add_argument('--canvas_h', type=int, default=0, help='canvas height in pixels (0: resolution_h, no canvas)')
    p.add_argument('--canvas_w', type=int, default=0, help='canvas width in pixels (0: resolution_w, no canvas)')
    p.add_argument('--window_overlap', type=int, default=-1, help='minimum overlap of neighbouring windows in pixels (default: half the smaller window side)')
    p.add_argument('--solver', type=str, default='ddim', choices=['ddim', 'dpmpp2m'],
                   help='dpmpp2m: second-order multistep steps on the blended Tweedie estimate behind the first timestep (ddim: the reference\'s steps)')
    p.add_argument('--guidance_rescale', type=float, default=0.0,
                   help='PHI in [0, 1]: scale every guided prediction back towards the standard deviation of its conditional one '
                        '(0: off; 0.7 is the value of arXiv:2305.08891)')
    p.add_argument('--eta', type=float, default=0.0,
                   help='E in [0, 1]: noise added by every trajectory step, generated inside the step kernel from (seed, step, canvas coordinate). '
                        '--solver ddim: the DDIM paper\'s eta; --solver dpmpp2m: k-diffusion\'s SDE-DPM-Solver++(2M) eta; the two coincide at 0 and 1 '
                        'and differ in between (0: off)')
    p.add_argument('--guidance_interval', type=str, default='',
                   help='T_HI,T_LO: integer timesteps, 1000 >= T_HI >= T_LO >= 0; trajectory steps at timesteps outside [T_LO, T_HI] use the '
                        'conditional prediction alone and run the UNet without the unconditional row (default: every step is guided)')
    p.add_argument('--apg', action='store_true',
                   help='adaptive projected guidance (arXiv:2410.02416): guidance on the Tweedie estimates, the part of the update parallel to the '
                        'conditional estimate scaled by --apg_eta, the update\'s norm clipped at --apg_norm (default: off)')
    p.add_argument('--apg_eta', type=float, default=0.0, help='ETA in [0, 1]: weight of the parallel part of the update under --apg (0: dropped; 1: CFG)')
    p.add_argument('--apg_norm', type=float, default=0.0, help='R >= 0: clip of the update\'s norm over one UNet row under --apg (0: no clip)')
    p.add_argument('--timestep_spacing', type=str, default='leading', choices=['leading', 'logsnr'],
                   help="logsnr: n_timesteps uniform in log-SNR from the 'leading' grid's first timestep down to t = 1")
    p.add_argument('--num_seeds', type=int, default=1, help='trajectories to sample: seeds seed..seed+n-1')
    p.add_argument('--seeds_per_batch', type=int, default=0, help='seeds co-batched into every UNet launch (0: all of this rank\'s seeds, at most 4)')
    p.add_argument('--gpus', type=int, default=1, help='shard the seeds over this many GPUs (one process per GPU, started by this script)')
    p.add_argument('--no_strict_reference', action='store_true',
                   help='route the concept weights for any concept count (the reference hooks only route when the UNet batch is 4, i.e. 3 concepts)')
    p.add_argument('--streams', type=int, default=1, help='launch chains per UNet call (2: batch rows split over two HIP streams)')
    p.add_argument('--lora_mode', type=str, default='merged', choices=['merged', 'lowrank'],
                   help='LoRA deltas as merged per-concept weight sets (default, fastest) or in the reference\'s own low-rank form up(down(x)) (no weight copies)')
    p.add_argument('--dtype', type=str, default='bf16', choices=['bf16', 'fp8'],
                   help='fp8: the transformer blocks\' projections, the attention outputs and the eligible ResnetBlock2D convolutions on e4m3 operands with power-of-two block scales (merged LoRA only)')
    p.add_argument('--no_graphs', action='store_true')
    p.add_argument('--tiny', action='store_true', help='tiny UNet config (smoke tests)')
    return p


def load_state_dict(path):
    if path.endswith('.safetensors'):
        from safetensors.torch import load_file
        return load_file(path)
    sd = torch.load(path, map_location='cpu')
    return sd.get('state_dict', sd)


def find_weights(folder, stem):
    """first existing of {stem}.fp16.safetensors / {stem}.safetensors / {stem}.bin under folder (or folder itself if a file)."""
    if os.path.isfile(folder):
        return folder
    for ext in ('.fp16.safetensors', '.safetensors', '.bin'):
        fp = os.path.join(folder, stem + ext)
        if os.path.exists(fp):
            return fp
    raise FileNotFoundError(f'no {stem}.[fp16.]safetensors/.bin under {folder}')


def save_png(img, path):
    """img [3,H,W] in [0,1] -> 8-bit PNG (image_processor.postprocess(..., 'pil') of fusion_sampling.py:526-527)."""
    from PIL import Image
    a = (img.clamp(0, 1).permute(1, 2, 0).float().cpu().numpy() * 255).round().astype('uint8')
    Image.fromarray(a).save(path)


def save_attention_outputs(opt, tw, side_dir, seeds):
    """--mask_source attention: the masks this rank used, under the side-car's file names '{side_dir}/{seg_concept}.jpg' (those of
    the last seed of the batch: like the side-car, every mask acquisition overwrites them), and with --save_attention_maps the raw
    per-level maps of every seed as attention_maps_{seed}_level{l}.npy ([n_tok, h_l, w_l], token order of --mask_token_ids) and, with
    --attn_mask_propagate, the propagated ones beside them as attention_maps_{seed}_level{l}_prop.npy"""
    import numpy as np
    from PIL import Image
    os.makedirs(side_dir, exist_ok=True)
    names = [c for c in opt.seg_concepts.split('+') if c]
    imgs = tw.mask_images[len(seeds) - 1]
    if len(names) != len(imgs):
        names = [f'concept{i}' for i in range(len(imgs))]
    for name, m in zip(names, imgs):
        Image.fromarray(m).save(os.path.join(side_dir, name + '.jpg'))
    if opt.save_attention_maps:
        for sd_, per in zip(seeds, tw.attention_maps):
            for lvl, m in per.items():
                np.save(os.path.join(side_dir, f'attention_maps_{sd_}_level{lvl}.npy'), m)
        for sd_, per in zip(seeds, tw.propagated_maps or []):
            for lvl, m in per.items():
                np.save(os.path.join(side_dir, f'attention_maps_{sd_}_level{lvl}_prop.npy'), m)


def output_stem(prompt_orig):
    """the '{prompt_orig}' of the output file names (fusion_sampling.py:526).  A file name holds 255 bytes, which a --long_prompts scene
    prompt exceeds: a stem over 200 bytes is cut to its first 160 characters (shortened further until they fit) plus 8 hex digits of the
    whole prompt's SHA-1.  Every name that could be written before is unchanged."""
    stem = prompt_orig.split('+')[0] or 'sample'
    if len(stem.encode('utf-8')) <= 200:
        return stem
    import hashlib
    head = stem[:160]
    while len(head.encode('utf-8')) > 190:
        head = head[:-1]
    return head + '_' + hashlib.sha1(stem.encode('utf-8')).hexdigest()[:8]


def noise_for_seed(seed, h, w):
    """x_T of one trajectory, drawn on the CPU like fusion_sampling.py:488 after seed_everything(seed) (utils_custom.py:10-14
    seeds torch's global generator; a fresh generator with the same seed yields the same first draw)."""
    return torch.randn(1, 4, h, w, generator=torch.Generator().manual_seed(int(seed)))


def keep_noise_for_seed(seed, h, w):
    """the fixed noise of a seed's kept region: the SECOND tensor of that seed's generator, behind its x_T (noise_for_seed), so that a
    seed's x_T is what it is without a keep region"""
    g = torch.Generator().manual_seed(int(seed))
    torch.randn(1, 4, h, w, generator=g)
    return torch.randn(1, 4, h, w, generator=g)


def parse_reroll(spec, seg_concepts):
    """'a dog+0' with --seg_concepts 'a cat+a dog' -> [0, 1]: every entry is one of the phrases or a 0-based index into them"""
    names = [c for c in seg_concepts.split('+') if c]
    out = []
    for e in (e.strip() for e in spec.split('+')):
        if e in names and e:
            i = names.index(e)
        elif e.isdigit() and int(e) < len(names):
            i = int(e)
        else:
            raise SystemExit(f"--reroll {spec!r}: {e!r} is neither one of the --seg_concepts phrases {names} nor an index below {len(names)}")
        if i in out:
            raise SystemExit(f"--reroll {spec!r}: region {i} ({names[i]!r}) is named twice")
        out.append(i)
    return sorted(out)


def keep_weight(masks, reroll, soft=None):
    """[1,1,h,w] weight of the KEPT part from the blend masks [K,1,h,w] (masks.build_masks: foreground masks, then the background):
    1 - min(1, sum of the re-rolled regions' foreground masks); with soft = (feather, dilate) in latent pixels that union is dilated and
    feathered first (masks.soft_region; (0, 0) gives the same bits)"""
    union = masks[list(reroll)].sum(dim=0, keepdim=True).clamp(max=1.0)
    if soft is not None:
        from tweediemix_amd import masks as M
        union = M.soft_region(union, soft[0], soft[1], device=masks.device)
    return (1.0 - union).contiguous()


def check_propagate_args(opt):
    """--attn_mask_propagate: 0..3 rounds, and only where the masks come from the attention maps (before anything touches the GPU)"""
    n = opt.attn_mask_propagate
    if not 0 <= n <= 3:
        raise SystemExit(f'--attn_mask_propagate {n}: 0..3 rounds through the self-attention')
    if n and opt.mask_source != 'attention':
        raise SystemExit(f'--attn_mask_propagate {n} refines the masks of --mask_source attention: it needs that mask source')


def check_shape_args(opt):
    """--attn_mask_shape / --attn_mask_keep_holes: only where the masks come from the attention maps, and holes are kept only in free-form
    masks (before anything touches the GPU)"""
    if opt.attn_mask_shape != 'rect' and opt.mask_source != 'attention':
        raise SystemExit(f'--attn_mask_shape {opt.attn_mask_shape} shapes the masks of --mask_source attention: it needs that mask source')
    if opt.attn_mask_keep_holes and opt.mask_source != 'attention':
        raise SystemExit('--attn_mask_keep_holes applies to the masks of --mask_source attention: it needs that mask source')
    if opt.attn_mask_keep_holes and opt.attn_mask_shape != 'free':
        raise SystemExit('--attn_mask_keep_holes keeps the holes of free-form masks: it needs --attn_mask_shape free (a rectangle has none)')


def check_soft_args(opt):
    """(mask_soften dict or None, (feather, dilate) of the keep region in latent pixels or None); refuses bad numbers and --reroll_* flags
    without a keep region (before anything touches the GPU).  The flags are image pixels, the kernels take latent pixels: / 8."""
    import math
    for flag, v in (('--mask_feather', opt.mask_feather), ('--reroll_feather', opt.reroll_feather)):
        if not (math.isfinite(v) and v >= 0):
            raise SystemExit(f'{flag} {v}: the width of the ramp in image pixels, a finite number >= 0')
    for flag, v in (('--mask_dilate', opt.mask_dilate), ('--reroll_dilate', opt.reroll_dilate)):
        if not math.isfinite(v):
            raise SystemExit(f'{flag} {v}: a finite number of image pixels (negative shrinks the region)')
    if (opt.reroll_feather or opt.reroll_dilate) and not (opt.keep_latents or opt.keep_image):
        raise SystemExit(f'--reroll_feather {opt.reroll_feather} / --reroll_dilate {opt.reroll_dilate} soften the border of a keep region: '
                         f'they need --keep_latents or --keep_image')
    soften = None
    if opt.mask_feather or opt.mask_dilate or opt.mask_normalize:
        soften = dict(feather=opt.mask_feather / 8.0, dilate=opt.mask_dilate / 8.0, normalize=bool(opt.mask_normalize))
    reroll = (opt.reroll_feather / 8.0, opt.reroll_dilate / 8.0) if (opt.reroll_feather or opt.reroll_dilate) else None
    return soften, reroll


def save_soft_weights(opt, tw, side_dir):
    """the soft foreground weights this rank used (those of the last mask set acquired: like the side-car's own files, every acquisition
    overwrites them) as 8-bit '{side_dir}/{seg_concept}_soft.png', on the grid the masks were built on"""
    import numpy as np
    from PIL import Image
    wts = tw.soft_weights
    if wts is None:
        return
    wts = (wts if wts.dim() == 4 else wts[-1])[:-1, 0].cpu().numpy()
    os.makedirs(side_dir, exist_ok=True)
    names = [c for c in opt.seg_concepts.split('+') if c]
    if len(names) != len(wts):
        names = [f'concept{i}' for i in range(len(wts))]
    for name, m in zip(names, wts):
        Image.fromarray(np.round(m * 255.0).astype(np.uint8)).save(os.path.join(side_dir, name + '_soft.png'))


def check_solver_args(opt):
    """--solver / --timestep_spacing / --guidance_rescale / --eta / --guidance_interval / --apg: refuses what the sampler would refuse, before
    anything touches the GPU.  opt.guidance_interval becomes None or (t_hi, t_lo), opt.apg None or dict(eta, norm_threshold)."""
    from tweediemix_amd.guidance import validate_interval
    try:
        opt.guidance_interval = validate_interval(opt.guidance_interval or None, '--guidance_interval')
    except ValueError as e:
        raise SystemExit(str(e))
    if opt.guidance_interval is not None and (opt.keep_latents or opt.keep_image):
        flag = '--keep_latents' if opt.keep_latents else '--keep_image'
        raise SystemExit(f'--guidance_interval {opt.guidance_interval[0]},{opt.guidance_interval[1]} does not combine with {flag}: '
                         f'the keep region exists on the guided step only')
    from tweediemix_amd.solver import validate_eta
    try:
        eta = validate_eta(opt.eta, '--eta')
    except ValueError as e:
        raise SystemExit(str(e))
    if eta > 0.0 and (opt.keep_latents or opt.keep_image):
        flag = '--keep_latents' if opt.keep_latents else '--keep_image'
        raise SystemExit(f'--eta {eta} does not combine with {flag}: the keep region exists on the deterministic step only')
    if opt.solver != 'ddim' and (opt.keep_latents or opt.keep_image):
        flag = '--keep_latents' if opt.keep_latents else '--keep_image'
        raise SystemExit(f'--solver {opt.solver} does not combine with {flag}: the keep region exists on the --solver ddim step only')
    from tweediemix_amd.guidance import validate_phi
    try:
        phi = validate_phi(opt.guidance_rescale, '--guidance_rescale')
    except ValueError as e:
        raise SystemExit(str(e))
    if phi > 0.0 and (opt.keep_latents or opt.keep_image):
        flag = '--keep_latents' if opt.keep_latents else '--keep_image'
        raise SystemExit(f'--guidance_rescale {phi} does not combine with {flag}: the keep region exists on the unscaled step only')
    # --apg: opt.apg becomes None or dict(eta, norm_threshold), what Tweediemix(apg=...) takes
    from tweediemix_amd.guidance import validate_apg
    if not opt.apg:
        if opt.apg_eta != 0.0 or opt.apg_norm != 0.0:
            raise SystemExit(f'--apg_eta {opt.apg_eta} / --apg_norm {opt.apg_norm} set the adaptive projected guidance of --apg: give --apg too')
        opt.apg = None
    else:
        try:
            opt.apg = validate_apg(dict(eta=opt.apg_eta, norm_threshold=opt.apg_norm), '--apg')
        except ValueError:
            raise SystemExit(f'--apg_eta {opt.apg_eta} --apg_norm {opt.apg_norm}: ETA in [0, 1] and R >= 0 (0: no clip), both finite')
        if phi > 0.0:
            raise SystemExit(f'--apg does not combine with --guidance_rescale {phi}: both re-shape the guided prediction and no order between them is defined')
        if opt.keep_latents or opt.keep_image:
            flag = '--keep_latents' if opt.keep_latents else '--keep_image'
            raise SystemExit(f'--apg does not combine with {flag}: the keep region exists on the step without adaptive projected guidance only')
    if opt.timestep_spacing == 'logsnr':
        from tweediemix_amd.schedule import Schedule
        try:
            Schedule(opt.n_timesteps, spacing='logsnr')
        except ValueError as e:
            raise SystemExit(f'--timestep_spacing logsnr with --n_timesteps {opt.n_timesteps}: {e}')


def check_keep_args(opt):
    """None for a run without a keep region, else dict(reroll=[indices], latent=[1,4,h,w] or None, image=PIL RGB or None); refuses what
    such a run cannot do (before anything touches the GPU)."""
    if not (opt.keep_latents or opt.keep_image):
        if opt.reroll:
            raise SystemExit('--reroll names the regions to sample anew inside a kept image: it needs --keep_latents or --keep_image')
        return None
    if opt.keep_latents and opt.keep_image:
        raise SystemExit('--keep_latents and --keep_image are mutually exclusive: one kept image per run')
    flag = '--keep_latents' if opt.keep_latents else '--keep_image'
    if not opt.mask_paths:
        raise SystemExit(f'{flag} needs --mask_paths: the kept region must be known before the first step '
                         f'(masks acquired during the run -- side-car, --mask_source attention, --random_masks -- come too late)')
    if not opt.reroll:
        raise SystemExit(f"{flag} needs --reroll: which of the --seg_concepts regions to sample anew (e.g. --reroll 1)")
    reroll = parse_reroll(opt.reroll, opt.seg_concepts)
    n_masks = len(opt.mask_paths.split('+'))
    if max(reroll) >= n_masks:
        raise SystemExit(f'--reroll {opt.reroll!r}: region {max(reroll)} has no mask, --mask_paths holds {n_masks}')
    path = opt.keep_latents or opt.keep_image
    if not os.path.isfile(path):
        raise SystemExit(f'{flag} {path!r}: no such file')
    h, w = opt.resolution_h // 8, opt.resolution_w // 8
    keep = dict(reroll=reroll, latent=None, image=None)
    if opt.keep_latents:
        lat = torch.load(path, map_location='cpu')
        if not (torch.is_tensor(lat) and tuple(lat.shape) == (1, 4, h, w)):
            got = tuple(lat.shape) if torch.is_tensor(lat) else type(lat).__name__
            raise SystemExit(f'--keep_latents {path!r} holds {got}; this run (resolution {opt.resolution_w} x {opt.resolution_h}) needs a [1, 4, {h}, {w}] latent')
        keep['latent'] = lat.float()
    else:
        if not (opt.vae_path or (opt.sd_path and os.path.isdir(os.path.join(opt.sd_path, 'vae'))) or (opt.synthetic and opt.tiny)):
            raise SystemExit('--keep_image needs the VAE encoder: give --vae_path (or --sd_path with a vae/ folder)')
        from PIL import Image
        im = Image.open(path)
        if im.size != (opt.resolution_w, opt.resolution_h):
            raise SystemExit(f'--keep_image {path!r} is {im.size[0]} x {im.size[1]}; it must be exactly resolution_w x resolution_h = '
                             f'{opt.resolution_w} x {opt.resolution_h}')
        keep['image'] = im.convert('RGB')
    return keep


def check_canvas_args(opt):
    """None for a run without a canvas (no flags, or a canvas of the window's size), else dict(height, width, overlap, n_win) in pixels; refuses
    what a canvas run cannot do (before anything touches the GPU)."""
    if not (opt.canvas_h or opt.canvas_w):
        if opt.window_overlap >= 0:
            raise SystemExit('--window_overlap is the overlap of the windows of a canvas: it needs --canvas_h or --canvas_w')
        return None
    from tweediemix_amd import canvas as CV
    rh, rw = opt.resolution_h, opt.resolution_w
    H, Wd = opt.canvas_h or rh, opt.canvas_w or rw
    if H % 8 or Wd % 8:
        raise SystemExit(f'--canvas_h {H} / --canvas_w {Wd}: canvas sizes are multiples of 8 pixels (the latent grid)')
    if H < rh or Wd < rw:
        raise SystemExit(f'--canvas_h {H} / --canvas_w {Wd}: the canvas is smaller than the window resolution_w x resolution_h = {rw} x {rh}')
    ov = opt.window_overlap if opt.window_overlap >= 0 else (min(rh, rw) // 2) // 8 * 8
    if ov % 8 or not 0 <= ov < min(rh, rw):
        raise SystemExit(f'--window_overlap {ov}: a multiple of 8 pixels below the window size {min(rh, rw)}')
    n_win = len(CV.window_layout(H // 8, Wd // 8, rh // 8, rw // 8, ov // 8))
    if n_win > 8:
        raise SystemExit(f'--canvas_h {H} / --canvas_w {Wd} with --window_overlap {ov}: {n_win} windows of {rw} x {rh}, at most 8 share a UNet launch')
    if n_win == 1:
        return None
    if opt.keep_latents or opt.keep_image or opt.reroll:
        raise SystemExit('--keep_latents / --keep_image / --reroll do not combine with a canvas: reconciling the windows would change the kept bits')
    if opt.mask_source == 'attention' and not (opt.mask_paths or opt.random_masks):
        raise SystemExit('--mask_source attention does not combine with a canvas: the token maps come per window and are not stitched')
    if opt.streams != 1:
        raise SystemExit(f'--streams {opt.streams}: a canvas runs on one launch chain (--streams 1)')
    if opt.seeds_per_batch and opt.seeds_per_batch * n_win > 8:
        raise SystemExit(f'--seeds_per_batch {opt.seeds_per_batch} x {n_win} windows = {opt.seeds_per_batch * n_win} co-batched row sets, at most 8')
    return dict(height=H, width=Wd, overlap=ov, n_win=n_win)


def default_seeds_per_batch(n_seeds, n_win=1):
    """seeds co-batched into every UNet launch when --seeds_per_batch is not given: all of this rank's seeds, at most 4; on a canvas of
    n_win windows as many as keep seeds x windows within the 8 co-batched row sets"""
    if n_win == 1:
        return min(max(n_seeds, 1), 4)
    return max(1, min(n_seeds, 8 // n_win))


def encode_keep_image(image, vae, scaling_factor, device, synthetic=False):
    """the kept latent of --keep_image: the VAE encoder's MEAN times the factor decode_final divides by (deterministic: no sample is drawn)"""
    from tweediemix_amd import vae as V, video as VI
    vcfg, sd = vae
    if 'encoder.conv_in.weight' not in sd:
        if not synthetic:
            raise SystemExit('--keep_image: the VAE weights hold no encoder (encoder.* / quant_conv.*)')
        sd = V.synthetic_state_dict(vcfg, encoder=True)
    plan = V.VAEEncoderPlan(vcfg, sd, 1, image.size[1], image.size[0], device)
    mean, _logvar = plan(VI.vae_pixel_values(image).to(device))
    return mean * scaling_factor


def parse_token_ids(spec):
    """'4,5+7' -> [[4, 5], [7]]"""
    try:
        out = [[int(p) for p in c.split(',') if p.strip()] for c in spec.split('+')]
    except ValueError:
        raise SystemExit(f"--mask_token_ids {spec!r}: '+'-separated concepts of ','-separated integer positions")
    if not out or any(not c for c in out):
        raise SystemExit(f"--mask_token_ids {spec!r}: every concept needs at least one position")
    return out


def attention_token_ids(opt, tokenizer):
    """token positions per foreground concept for --mask_source attention"""
    if opt.mask_token_ids:
        return parse_token_ids(opt.mask_token_ids)
    if tokenizer is None:
        raise SystemExit('--mask_source attention without a tokenizer (--text_embeds_path / --synthetic) needs --mask_token_ids')
    from tweediemix_amd import text as T
    prompt = opt.prompt_orig.split('+')[0]
    try:
        if opt.long_prompts:          # positions in the concatenated chunks; `tokenizer` is then the list the prompts were cut with
            return [T.token_positions_long(tokenizer, prompt, ph) for ph in opt.seg_concepts.split('+')]
        return [T.phrase_token_positions(tokenizer, prompt, ph) for ph in opt.seg_concepts.split('+')]
    except ValueError as e:
        raise SystemExit(f'--mask_source attention: {e}')


def check_long_prompt_args(opt):
    if opt.synthetic_chunks != 1 and not (opt.long_prompts and opt.synthetic):
        raise SystemExit('--synthetic_chunks belongs to --synthetic --long_prompts')
    if not 1 <= opt.synthetic_chunks <= 3:
        raise SystemExit(f'--synthetic_chunks {opt.synthetic_chunks}: 1..3 chunks of 77 keys')


def check_long_embeds(opt, te, ts):
    """--long_prompts: both embedding sets hold 77 c keys, the same c in 1..3; returns the key count"""
    Lk = te[0].shape[1]
    if Lk not in (77, 154, 231) or ts[0].shape[1] != Lk:
        raise SystemExit(f'--long_prompts: text embeddings of {Lk} and {ts[0].shape[1]} keys; both sets need 77 c keys, the same c in 1..3')
    return Lk


def main(argv=None):
    opt = build_parser().parse_args(argv)
    check_long_prompt_args(opt)
    if opt.dtype == 'fp8' and opt.lora_mode == 'lowrank':
        raise SystemExit('--dtype fp8 quantises the merged per-concept projection weights: use --lora_mode merged')
    check_propagate_args(opt)
    check_shape_args(opt)
    soften, reroll_soft = check_soft_args(opt)
    canvas = check_canvas_args(opt)
    keep = check_keep_args(opt)
    check_solver_args(opt)
    from tweediemix_amd import dist as D, launch as LA, masks as M, sampler as S, unet as U, weights as Wt
    if opt.gpus > 1 and not LA.launched():
        return LA.self_launch(opt.gpus)
    rank, local, world = LA.rank_env()
    if world > 1:
        single = bool(os.environ.get('TMIX_SINGLE_GPU_DIST_TEST'))      # tests: all ranks on GPU 0, gloo
        opt.device = 'cuda:0' if single else f'cuda:{local}'
        torch.cuda.set_device(torch.device(opt.device))
        # through dist.init like bench.py: a rendezvous port stolen between the launcher's probe and the bind exits with EADDRINUSE_RC,
        # which launch.self_launch retries on a fresh port
        D.init(torch.device(opt.device), world, backend='gloo' if single else None)
    say = print if rank == 0 else (lambda *a, **k: None)
    if opt.sd_version != 'xl':
        say(f"note: --sd_version {opt.sd_version}: like the reference (fusion_sampling.py:119) only the SDXL pipeline exists")
    concepts = [c for c in opt.concepts.split('+') if c] or ['a', 'b', 'background']
    K = len(concepts)                                    # concept_num, background last (fusion_sampling.py:143-148)
    cfg = U.TINY if opt.tiny else U.SDXL
    if opt.sd_path and os.path.exists(os.path.join(opt.sd_path, 'unet', 'config.json')):
        import json
        cfg = U.UNetConfig.from_diffusers(json.load(open(os.path.join(opt.sd_path, 'unet', 'config.json'))))
    kind = 'lora' if LORA else 'custom'
    S.seed_everything(opt.seed)
    tokenizer = None
    if opt.synthetic:
        sd = Wt.synthetic_state_dict(cfg, seed=1234, device=opt.device, dtype=torch.bfloat16)
        con = Wt.synthetic_concepts(cfg, kind, K, device=opt.device)
        g = torch.Generator().manual_seed(42)
        Lk = 77 * opt.synthetic_chunks                   # (1 without --long_prompts: the draws below are then today's)
        te = (torch.randn(K + 2, Lk, cfg.cross_dim, generator=g), torch.randn(K + 2, cfg.pooled_dim, generator=g))
        ts = (torch.randn(K, Lk, cfg.cross_dim, generator=g), torch.randn(K, cfg.pooled_dim, generator=g))
    else:
        unet_file = opt.unet_path or (opt.sd_path and find_weights(os.path.join(opt.sd_path, 'unet'), 'diffusion_pytorch_model'))
        if not (unet_file and (opt.text_embeds_path or opt.sd_path) and opt.personal_checkpoint):
            sys.exit("need --personal_checkpoint and either --sd_path (local diffusers-layout SDXL checkpoint) or "
                     "--unet_path + --text_embeds_path (or --synthetic); there is no HF hub download here")
        sd = load_state_dict(unet_file)
        sts = [torch.load(p, map_location='cpu') for p in opt.personal_checkpoint.split('+')]            # :156-157
        con = [st['unet'] for st in sts]
        if opt.text_embeds_path:
            emb = torch.load(opt.text_embeds_path, map_location='cpu')
            te, ts = emb['text_embeds'], emb['text_embeds_single']
        else:
            from tweediemix_amd import text as T
            tpath = T.TextPath(opt.sd_path, opt.device)
            te, ts, K_text = tpath.embed(opt, sts)
            tokenizer = tpath.tokenizers if opt.long_prompts else tpath.tokenizers[0]
            assert K_text == K, (K_text, K)
    if opt.long_prompts:
        n_keys = check_long_embeds(opt, te, ts)
    W = U.UNetWeights(cfg, sd, opt.device, (kind, con), lora_mode=opt.lora_mode)
    out_h, out_w = (canvas['height'], canvas['width']) if canvas else (opt.resolution_h, opt.resolution_w)      # what the files hold
    h, w = out_h // 8, out_w // 8                        # the grid of x_T, the masks and the results: the canvas's, where there is one
    sidecar = False
    attn = None
    if opt.mask_paths:
        fg = opt.mask_paths.split('+')
    elif opt.random_masks:
        fg = None
    elif opt.mask_source == 'attention':              # in-process masks: the provider below is never called
        fg = None
        attn = dict(tokens=attention_token_ids(opt, tokenizer), threshold=opt.attn_mask_threshold, propagate=opt.attn_mask_propagate,
                    shape=opt.attn_mask_shape, fill_holes=not opt.attn_mask_keep_holes)
        if opt.long_prompts and max(p for c in attn['tokens'] for p in c) >= n_keys:
            raise SystemExit(f"--mask_token_ids: positions up to {n_keys - 1} ({n_keys // 77} chunks of 77 keys)")
        side_dir = M.sidecar_layout(opt.output_path, rank, world, local, opt.seg_gpu)[0]
    elif opt.synthetic:
        fg = None                                        # seeded rectangles, one set per trajectory seed (drawn when the sampler asks)
    else:   # the reference's file contract (:453-466): the side-car writes '<seg_concept>.jpg' under output_path
        # (several ranks: one side-car directory per rank, see masks.sidecar_layout)
        side_dir, side_gpu = M.sidecar_layout(opt.output_path, rank, world, local, opt.seg_gpu)
        fg = [os.path.join(side_dir, sp + '.jpg') for sp in opt.seg_concepts.split('+')]
        sidecar = True
    vae, vae_scaling = None, None
    vae_dir = opt.vae_path or (opt.sd_path and os.path.isdir(os.path.join(opt.sd_path, 'vae')) and os.path.join(opt.sd_path, 'vae'))
    if vae_dir:
        from tweediemix_amd import vae as V
        vcfg = V.FULL
        if os.path.isdir(vae_dir) and os.path.exists(os.path.join(vae_dir, 'config.json')):
            import json
            j = json.load(open(os.path.join(vae_dir, 'config.json')))
            vcfg = dict(block_out_channels=tuple(j['block_out_channels']), layers_per_block=j.get('layers_per_block', 2),
                        latent_channels=j.get('latent_channels', 4), out_channels=j.get('out_channels', 3),
                        groups=j.get('norm_num_groups', 32))
            vae_scaling = j.get('scaling_factor')
        vae = (vcfg, load_state_dict(find_weights(vae_dir, 'diffusion_pytorch_model')))
    elif opt.synthetic and opt.tiny:
        from tweediemix_amd import vae as V
        vae = (V.TINY, V.synthetic_state_dict(V.TINY))
    seeds = D.seed_shard([opt.seed + i for i in range(opt.num_seeds)], rank, world)
    per = opt.seeds_per_batch or default_seeds_per_batch(len(seeds), canvas['n_win'] if canvas else 1)
    strict = not opt.no_strict_reference
    if strict and K + 1 != 4 and kind in ('custom', 'lora'):
        say(f"note: {K} concepts -> UNet batch {K + 1}: the reference's attention hooks only route concept weights when the batch is 4 "
            f"(utils_custom.py:62, utils_lora.py:63), so like the reference this run uses the BASE weights for every row; "
            f"--no_strict_reference routes them")
    current = {"ids": [opt.seed], "turn": 0}             # the seeds of the batch being sampled; the sampler asks once per seed, in order

    def provider(x0):
        if fg is not None:
            return M.build_masks(fg, h, w, opt.device)
        sd_ = current["ids"][current["turn"] % len(current["ids"])]
        current["turn"] += 1
        return M.build_masks(M.random_rectangle_masks(K, out_h, out_w, seed=sd_), h, w, opt.device)

    tw = S.Tweediemix(opt, W, te, ts, provider, concept_num=K, lora=LORA,
                      strict_reference=strict, use_graphs=not opt.no_graphs, n_seeds=per, n_streams=opt.streams, vae=vae,
                      fp8=(opt.dtype == 'fp8'), attention_masks=attn, mask_soften=soften,
                      solver=opt.solver, timestep_spacing=opt.timestep_spacing, guidance_rescale=opt.guidance_rescale,
                      eta=opt.eta, noise_seeds=([opt.seed] * per if opt.eta > 0.0 else None), guidance_interval=opt.guidance_interval,
                      **(dict(apg=opt.apg) if opt.apg else {}),
                      **(dict(canvas={k: canvas[k] for k in ('height', 'width', 'overlap')}) if canvas else {}))
    if vae_scaling:                                       # fusion_sampling.py:518 divides by vae.config.scaling_factor
        tw.vae_scaling_factor = float(vae_scaling)
    if sidecar and vae is not None:
        # with a VAE the whole contract runs like the reference: decode the Tweedie preview to {output_path}/tweedie.jpg,
        # call `CUDA_VISIBLE_DEVICES={seg_gpu} python text_segment/run_expand.py ...` (TMIX_SEG_CMD overrides the command),
        # read the masks back; without one the mask files must already be there
        tw.mask_provider = M.SidecarMaskProvider(tw, side_dir, opt.seg_concepts, seg_gpu=side_gpu,
                                                 cmd_template=os.environ.get('TMIX_SEG_CMD'))
    if keep is not None:                                  # one kept latent and one weight, shared by every seed of every batch
        keep_x0 = keep['latent'] if keep['latent'] is not None else \
            encode_keep_image(keep['image'], vae, tw.vae_scaling_factor, opt.device, synthetic=opt.synthetic)
        keep_w = keep_weight(M.build_masks(fg, h, w, opt.device), keep['reroll'], reroll_soft)
    lats, imgs = [], []
    for b0 in range(0, len(seeds), per):
        batch = seeds[b0:b0 + per]
        ids = (batch + batch * per)[:per]                # a ragged last batch is padded with repeats and trimmed below
        current["ids"], current["turn"] = ids, 0
        if keep is not None:
            tw.set_keep(keep_x0, keep_w, torch.cat([keep_noise_for_seed(sd_, h, w) for sd_ in ids]))
        if opt.eta > 0.0:                                 # a trajectory's step noise is a function of its own seed, as its x_T is
            tw.set_noise_seeds(ids)
        lat_b = tw.run_fusion(torch.cat([noise_for_seed(sd_, h, w) for sd_ in ids]))
        lats.append(lat_b[:len(batch)])
        if attn is not None:
            save_attention_outputs(opt, tw, side_dir, batch)
        if soften is not None:
            save_soft_weights(opt, tw, M.sidecar_layout(opt.output_path, rank, world, local, opt.seg_gpu)[0])
        if vae is not None:                               # fusion_sampling.py:496-528
            imgs.append(tw.decode_final(lat_b)[:len(batch)])
    dev = torch.device(opt.device)
    lat = torch.cat(lats) if lats else torch.zeros(0, 4, h, w, device=dev)
    img = torch.cat(imgs) if imgs else None
    if world > 1:                                         # the result gather: the only collective of this path
        import torch.distributed as dist
        lat = D.gather_latents(lat.contiguous(), opt.num_seeds, rank, world)
        if vae is not None:
            img = D.gather_latents(img.contiguous() if img is not None else torch.zeros(0, 3, out_h, out_w, device=dev),
                                   opt.num_seeds, rank, world)
    if rank == 0:
        os.makedirs(opt.output_path_all, exist_ok=True)
        prompt_orig = output_stem(opt.prompt_orig)
        for i in range(opt.num_seeds):
            out = f'{opt.output_path_all}/{prompt_orig}_{opt.seed + i}.latent.pt'
            torch.save(lat[i:i + 1].cpu(), out)
            print('saved', out)
            if vae is not None:
                out = f'{opt.output_path_all}/{prompt_orig}_{opt.seed + i}.png'
                save_png(img[i], out)
                print('saved', out)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    return lat


if __name__ == '__main__':
    rc = main()
    sys.exit(rc if isinstance(rc, int) else 0)
