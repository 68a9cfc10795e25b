"""GPU: many videos per UNet call (tweediemix_amd.video.VideoSampler, i2vgen.I2VVideoPlan, run_video.py's batched path).
The two step kernels against tmix_vpred_step and a torch permute / copy, the sampler at S = 1 against the host loop, co-batched
videos against their own single runs, and the CLI (ragged batch, two images, two ranks) against single-video runs -- bit for bit --
plus the one-video run's --conditioning_path."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cli(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "run_video.py"))
    rv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rv)
    return rv


# ------------------------------------------------------------------------------------------------------------ 1. the kernels
@pytest.mark.timeout(60)
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("F", [2, 16])
@pytest.mark.parametrize("hw", [(8, 8), (7, 13)])
@pytest.mark.parametrize("streams", [2, 1])
def test_prologue_and_vpred_dev_match_vpred_step_in_one_graph(S, F, hw, streams):
    from tweediemix_amd import ops
    h, w = hw
    g = torch.Generator(device="cuda").manual_seed(S * 100 + F + h)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)
    if streams == 2:                                    # two chains of S clips
        x_in = [rnd(S * F, 8, h, w), rnd(S * F, 8, h, w)]
        t_dev = [torch.zeros(S, device="cuda"), torch.zeros(S, device="cuda")]
        eps = [rnd(S * F, 4, h, w), rnd(S * F, 4, h, w)]
        halves = [(x_in[i], t_dev[i], eps[i]) for i in range(2)]
    else:                                               # one plan of 2S clips, the text half from clip S on
        xi, td, ep = rnd(2 * S * F, 8, h, w), torch.zeros(2 * S, device="cuda"), rnd(2 * S * F, 4, h, w)
        halves = [(xi[i * S * F:(i + 1) * S * F], td[i * S:(i + 1) * S], ep[i * S * F:(i + 1) * S * F]) for i in range(2)]
    feat = [hv[0][:, 4:].clone() for hv in halves]
    x = rnd(S, 4, F, h, w)
    ref = x.clone()
    prm = torch.zeros(8, device="cuda")
    (xu, tu, eu), (xc, tc, ec) = halves

    def step():
        ops.video_step_prologue(x, xu, tu, xc, tc, prm)
        ops.vpred_step_dev(x, eu, ec, prm)

    acp = np.linspace(0.999, 0.01, 1000).astype(np.float32)
    prm.copy_(ops.video_step_params(981, 9.0, acp[981], acp[961]))
    step()                                               # warm-up (also: eager == reference below for the first step)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        step()
    pipe = lambda e: e.view(S, F, 4, h, w).permute(0, 2, 1, 3, 4)
    for k, (t, tn, gs) in enumerate(((981, 961, 9.0), (501, 481, 4.5), (21, 1, 1.25), (1, -19, 9.0))):
        if k:
            prm.copy_(ops.video_step_params(t, gs, acp[t], acp[tn] if tn >= 0 else acp[0]))
            gr.replay()
        before = ref.clone()
        for s in range(S):
            v = torch.cat([pipe(eu)[s:s + 1], pipe(ec)[s:s + 1]]).contiguous()
            ref[s:s + 1] = ops.vpred_step(before[s:s + 1].contiguous(), v, gs, acp[t], acp[tn] if tn >= 0 else acp[0])
        torch.cuda.synchronize()
        assert torch.equal(x, ref), (k, float((x - ref).abs().max()))
        for (xi_, ti_, _e), f in zip(halves, feat):
            assert torch.equal(xi_.view(S, F, 8, h, w)[:, :, :4], before.permute(0, 2, 1, 3, 4))
            assert torch.equal(xi_[:, 4:], f)           # the image-latent channels are never written
            assert torch.equal(ti_, torch.full_like(ti_, float(t)))


def test_step_kernels_report_argument_errors():
    from tweediemix_amd import lib as L, ops
    x = torch.zeros(2, 4, 2, 8, 8, device="cuda")
    short = torch.zeros(2 * 2, 4, 8, 8, device="cuda")                # rows of 4 channels: shorter than the 8-channel input rows
    prm = torch.zeros(8, device="cuda")
    t = torch.zeros(2, device="cuda")
    l = L.load()
    assert l.tmix_video_step_prologue(x.data_ptr(), short.data_ptr(), 100, t.data_ptr(), short.data_ptr(), 512, t.data_ptr(), prm.data_ptr(),
                                      2, 4, 2, 64, 4, None) == L.ESHAPE
    assert b"clip stride" in l.tmix_last_error_string()
    assert l.tmix_video_step_prologue(x.data_ptr(), short.data_ptr(), 512, None, short.data_ptr(), 512, t.data_ptr(), prm.data_ptr(),
                                      2, 4, 2, 64, 4, None) == L.EINVAL
    with pytest.raises(AssertionError):                               # 8-channel rows claimed over a 4-channel buffer: refused before the launch
        ops.video_step_prologue(x, short, t, short, t, prm, clip_stride_u=2 * 8 * 64, clip_stride_c=2 * 8 * 64)
    assert l.tmix_vpred_step_dev(x.data_ptr(), None, 512, short.data_ptr(), 512, prm.data_ptr(), 2, 4, 2, 64, None) == L.EINVAL
    assert l.tmix_vpred_step_dev(x.data_ptr(), short.data_ptr(), 512, short.data_ptr(), 512, prm.data_ptr(), 2, 4, 2, 0, None) == L.ESHAPE


# ------------------------------------------------------------------------------------------------------------ 2./3. the sampler
FR, H, W = 16, 16, 8


def _weights():
    from tweediemix_amd import i2vgen as I
    from tweediemix_amd.weights import synthetic_i2vgen_state_dict
    return I.I2VWeights(I.TINY, synthetic_i2vgen_state_dict(I.TINY))


def _video(seed):
    """one video's conditioning rows [2, ...] (uncond first) and x_T, as run_video.py --synthetic draws them"""
    g = torch.Generator().manual_seed(seed)
    c = dict(pe=torch.randn(2, 77, 128, generator=g), ie=torch.randn(2, 128, generator=g), il=torch.randn(2, 4, FR, H, W, generator=g))
    return c, torch.randn(1, 4, FR, H, W, generator=g)


def _schedule(n=10):
    from tweediemix_amd import video as V
    acp, kw = V.alphas_from_scheduler_config(dict(beta_schedule="squaredcos_cap_v2", rescale_betas_zero_snr=True, steps_offset=1, set_alpha_to_one=False))
    return V.VideoSchedule(acp, n, **kw)


def _batched(Wt, vids, streams, graphs=True, autotune=False):
    from tweediemix_amd import i2vgen as I, video as V
    S = len(vids)
    rows = lambda k: torch.cat([c[k][r:r + 1] for r in (0, 1) for c, _x in vids])
    fe, ctx, ilf = I.conditioning(Wt, torch.tensor([8.0] * 2 * S), rows("il"), rows("ie"), rows("pe"))
    plan = I.I2VVideoPlan(Wt, S, FR, H, W, fe, ctx, ilf, streams=streams, autotune=autotune)
    sch = _schedule()
    smp = V.VideoSampler(plan, sch, 9.0, V.FeatureInjector(sch.injection_schedule(0.2), 0.7, clips=2 * S, frames=FR), use_graphs=graphs)
    out = smp.sample(torch.cat([x for _c, x in vids]).cuda())
    assert len(smp.graphs) <= 2 and (len(smp.graphs) == 2) == graphs
    return out.cpu()


def _host_loop(Wt, vid, streams, graphs=True):
    """the reference-shaped host loop: V.sample_loop over I2VPlanGroup(clips=2) / I2VPlan(clips=2), one recorded graph per injection state."""
    from tweediemix_amd import i2vgen as I, video as V
    c, x = vid
    fe, ctx, ilf = I.conditioning(Wt, torch.tensor([8.0, 8.0]), c["il"], c["ie"], c["pe"])
    plan = (I.I2VPlanGroup if streams == 2 else I.I2VPlan)(Wt, 2, FR, H, W, fe, ctx, ilf, autotune=False)
    sch = _schedule()
    inj = V.FeatureInjector(sch.injection_schedule(0.2), 0.7, clips=2, frames=FR)
    cache = {}

    def unet(xin, t):
        plan.inject, plan.interp = V.injection_active(t, inj.schedule), inj.interp     # the plan carries the injection as ops of its forward
        if streams == 2:
            plan.set_input(xin, t)
        else:
            plan.x_in.view(2, FR, 8, H, W)[:, :, :4] = xin.permute(0, 2, 1, 3, 4)
            plan.t_dev.fill_(float(t))
        if not graphs:
            plan.run()
        else:
            gr = cache.get(plan.inject)
            if gr is None:
                plan.run(); torch.cuda.synchronize()
                gr = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gr):
                    plan.run()
                cache[plan.inject] = gr
            gr.replay()
        return plan.eps.view(2, FR, 4, H, W).permute(0, 2, 1, 3, 4).contiguous()

    return V.sample_loop(unet, x.cuda(), sch, 9.0, inj).cpu()


@pytest.mark.timeout(120)
@pytest.mark.parametrize("streams", [2, 1])
def test_sampler_one_video_equals_host_loop(streams):
    """10 steps, injection on the first two: the new sampler at S = 1 is V.sample_loop bit for bit, with and without graphs."""
    torch.manual_seed(0)
    Wt = _weights()
    vid = _video(3)
    for graphs in (True, False):
        a = _batched(Wt, [vid], streams, graphs)
        b = _host_loop(Wt, vid, streams, graphs)
        assert torch.equal(a, b), (graphs, float((a - b).abs().max()))


@pytest.mark.timeout(120)
def test_three_co_batched_videos_equal_their_single_runs(monkeypatch):
    """S = 3 videos with different images (conditioning) and seeds: each equals its own S = 1 run.  One tiling everywhere
    (TMIX_FORCE_TILE; see test_two_seeds_co_batched_equal_independent_runs): the S = 1 and S = 3 launches have different shape keys,
    and two tilings can add a row's LayerNorm statistics in another order."""
    monkeypatch.setenv("TMIX_FORCE_TILE", "1")
    Wt = _weights()
    vids = [_video(s) for s in (11, 12, 13)]
    many = _batched(Wt, vids, 2, autotune=True)
    for i, v in enumerate(vids):
        one = _batched(Wt, [v], 2, autotune=True)
        assert torch.equal(many[i:i + 1], one), (i, float((many[i:i + 1] - one).abs().max()))


# ------------------------------------------------------------------------------------------------------------ 4.-6. the CLI
COMMON = ["--synthetic", "--tiny", "--height", "128", "--width", "64", "--num_inference_steps", "10", "--injection_timestep", "0.2"]


def _single(rv, tmp_path, seed, extra=()):
    d = tmp_path / f"single_{seed}"
    rv.main(COMMON + ["--seed", str(seed), "--output_dir", str(d)] + list(extra))
    return torch.load(d / f"output_i2v_seed_{seed}.latent.pt")


@pytest.mark.timeout(120)
def test_cli_ragged_batch_equals_single_runs(tmp_path, monkeypatch):
    """--num_seeds 3 --seeds_per_batch 2: batches of 2 and 1 (+ 1 padding video); every file equals that of a single --seed run."""
    monkeypatch.setenv("TMIX_FORCE_TILE", "1")                         # same tiling for the S = 2 and the single runs' shapes
    rv = _cli("run_video_batch_cli4")
    lat = rv.main(COMMON + ["--seed", "3", "--num_seeds", "3", "--seeds_per_batch", "2", "--output_dir", str(tmp_path / "multi")])
    assert lat.shape == (3, 4, 16, 16, 8)
    for s in (3, 4, 5):
        a = torch.load(tmp_path / "multi" / f"output_i2v_seed_{s}.latent.pt")
        assert a.shape == (1, 4, 16, 16, 8) and torch.equal(a, _single(rv, tmp_path, s)), s


def _i2v_folder(tmp_path, golden_dir):
    """the synthetic diffusers-layout I2VGen-XL folder of test_i2vgen_gpu.test_run_video_from_image_and_prompt"""
    import json, shutil
    from safetensors.torch import save_file
    from tweediemix_amd import i2vgen as I, vae as V, weights as Wt
    ck = tmp_path / "i2v"
    (ck / "unet").mkdir(parents=True)
    save_file({k: v.contiguous() for k, v in Wt.synthetic_i2vgen_state_dict(I.TINY).items()}, str(ck / "unet" / "diffusion_pytorch_model.safetensors"))
    z = np.load(os.path.join(golden_dir, "clip_text.npz"))
    sd = {k[len("l") + 4:]: torch.from_numpy(z[k].astype(np.float32)) for k in z.files if k.startswith("l.sd.")}
    key = [k for k in sd if k.endswith("token_embedding.weight")][0]
    g = torch.Generator().manual_seed(1)
    sd[key] = torch.cat([sd[key], torch.randn(620 - 64, 128, generator=g) * 0.05])
    (ck / "text_encoder").mkdir()
    save_file({k: v.contiguous() for k, v in sd.items()}, str(ck / "text_encoder" / "model.safetensors"))
    json.dump({"hidden_act": "quick_gelu", "num_attention_heads": 2, "eos_token_id": 2}, open(ck / "text_encoder" / "config.json", "w"))
    shutil.copytree(os.path.join(golden_dir, "clip_tok"), ck / "tokenizer")
    zv = np.load(os.path.join(golden_dir, "clip_vision.npz"))
    vsd = {k[3:]: torch.from_numpy(zv[k].astype(np.float32)) for k in zv.files if k.startswith("sd.")}
    vsd["visual_projection.weight"] = torch.randn(128, 320, generator=g) * 320 ** -0.5
    (ck / "image_encoder").mkdir()
    save_file({k: v.contiguous() for k, v in vsd.items()}, str(ck / "image_encoder" / "model.safetensors"))
    json.dump({"image_size": 56, "patch_size": 14, "num_attention_heads": 4, "hidden_act": "gelu"}, open(ck / "image_encoder" / "config.json", "w"))
    (ck / "vae").mkdir()
    vae_sd = V.synthetic_state_dict(V.TINY, nontrivial=True)
    vae_sd.update(V.synthetic_state_dict(V.TINY, seed=9, nontrivial=True, encoder=True))
    save_file({k: v.contiguous() for k, v in vae_sd.items()}, str(ck / "vae" / "diffusion_pytorch_model.safetensors"))
    json.dump({"block_out_channels": list(V.TINY["block_out_channels"]), "layers_per_block": 1}, open(ck / "vae" / "config.json", "w"))
    return ck


@pytest.mark.timeout(180)
def test_cli_two_images_equal_single_image_runs(tmp_path, monkeypatch, golden_dir):
    """--image_path a.png+b.png with --vae_path: per image, the latent and the 16-frame GIF equal the single-image run's (both runs
    decode in batches of frames)."""
    from PIL import Image
    monkeypatch.setenv("TMIX_FORCE_TILE", "1")
    ck = _i2v_folder(tmp_path, golden_dir)
    imgs = []
    for i, shape in enumerate(((200, 300, 3), (150, 260, 3))):
        p = tmp_path / f"img{i}.png"
        Image.fromarray(np.random.RandomState(i).randint(0, 256, shape, dtype=np.uint8)).save(p)
        imgs.append(p)
    rv = _cli("run_video_batch_cli5")
    common = ["--i2v_path", str(ck), "--vae_path", str(ck / "vae"), "--tiny", "--height", "64", "--width", "128", "--num_inference_steps", "4",
              "--seed", "5", "--prompt", "a cat and a dog running", "--negative_prompt", "blurry"]
    rv.main(common + ["--image_path", f"{imgs[0]}+{imgs[1]}", "--output_dir", str(tmp_path / "both")])
    for i, p in enumerate(imgs):
        rv.main(common + ["--image_path", str(p), "--output_dir", str(tmp_path / f"one{i}")])
        a = torch.load(tmp_path / "both" / f"img{i}_seed_5.latent.pt")
        b = torch.load(tmp_path / f"one{i}" / "output_i2v_seed_5.latent.pt")
        assert a.shape == (1, 4, 16, 8, 16) and torch.equal(a, b), i
        ga, gb = Image.open(tmp_path / "both" / f"img{i}_seed_5.gif"), Image.open(tmp_path / f"one{i}" / "output_i2v_seed_5.gif")
        assert ga.n_frames == gb.n_frames == 16 and ga.size == gb.size == (128, 64)
        for f in range(16):
            ga.seek(f); gb.seek(f)
            fa, fb = np.asarray(ga.convert("RGB"), np.int16), np.asarray(gb.convert("RGB"), np.int16)
            assert np.array_equal(fa, fb), (i, f, int(np.abs(fa - fb).max()))


@pytest.mark.timeout(180)
def test_cli_conditioning_path_one_video(tmp_path, monkeypatch, golden_dir):
    """--conditioning_path on the one-video run: a file holding only the prompt embeddings the run computes gives the no-file latent
    bit for bit (the merge and the generator's draw order) without computing them; a file holding all three keys runs neither the
    text tower nor the image towers."""
    from PIL import Image
    monkeypatch.setenv("TMIX_FORCE_TILE", "1")
    ck = _i2v_folder(tmp_path, golden_dir)
    img = tmp_path / "img.png"
    Image.fromarray(np.random.RandomState(0).randint(0, 256, (200, 300, 3), dtype=np.uint8)).save(img)
    rv = _cli("run_video_batch_cli7")
    common = ["--i2v_path", str(ck), "--image_path", str(img), "--tiny", "--height", "64", "--width", "128", "--num_inference_steps", "4",
              "--seed", "5", "--prompt", "a cat and a dog running", "--negative_prompt", "blurry"]
    seen = {}

    def spy(name):
        fn = getattr(rv, name)
        def wrapped(*a, **k):
            seen[name] = fn(*a, **k)
            return seen[name]
        monkeypatch.setattr(rv, name, wrapped)

    def refuse(*a, **k):
        raise AssertionError("computed what the --conditioning_path file holds")

    for name in ("encode_prompt", "encode_images", "image_latents"):
        spy(name)
    want = rv.main(common + ["--output_dir", str(tmp_path / "plain")]).cpu()
    torch.save({"prompt_embeds": seen["encode_prompt"]}, tmp_path / "pe.pt")
    monkeypatch.setattr(rv, "encode_prompt", refuse)
    got = rv.main(common + ["--conditioning_path", str(tmp_path / "pe.pt"), "--output_dir", str(tmp_path / "pe")]).cpu()
    assert torch.equal(got, want), float((got - want).abs().max())
    assert torch.equal(torch.load(tmp_path / "pe" / "output_i2v_seed_5.latent.pt"), torch.load(tmp_path / "plain" / "output_i2v_seed_5.latent.pt"))
    emb = seen["encode_images"]["image_embeddings"]
    torch.save({"prompt_embeds": seen["encode_prompt"], "image_embeddings": torch.cat([torch.zeros_like(emb), emb]),
                "image_latents": seen["image_latents"]}, tmp_path / "all.pt")
    for name in ("encode_images", "image_latents"):
        monkeypatch.setattr(rv, name, refuse)
    lat = rv.main(common + ["--conditioning_path", str(tmp_path / "all.pt"), "--output_dir", str(tmp_path / "all")]).cpu()
    assert lat.shape == (1, 4, 16, 8, 16) and torch.isfinite(lat).all()


@pytest.mark.timeout(240)
def test_cli_two_ranks_equal_single_runs(tmp_path, monkeypatch):
    """run_video.py --gpus 2 --num_seeds 3 (two ranks started by the script on one GPU over gloo, videos sharded round-robin,
    latents gathered, rank 0 writes the files) gives every seed's single-run file bit for bit."""
    monkeypatch.setenv("TMIX_FORCE_TILE", "1")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(TMIX_SINGLE_GPU_DIST_TEST="1", TMIX_FORCE_TILE="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_video.py"), "--gpus", "2", "--num_seeds", "3", "--seed", "20",
                        "--output_dir", str(tmp_path / "sharded")] + COMMON, capture_output=True, text=True, timeout=200, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    rv = _cli("run_video_batch_cli6")
    for s in (20, 21, 22):
        a = torch.load(tmp_path / "sharded" / f"output_i2v_seed_{s}.latent.pt")
        assert torch.equal(a, _single(rv, tmp_path, s)), s
