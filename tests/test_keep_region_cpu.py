"""CPU: the command-line half of the keep region (--keep_latents / --keep_image / --reroll of fusion_generation/fusion_sampling.py) and
the ctypes declaration of tmix_fused_tweedie_step_keep_dev against its prototype in include/tmix.h.  Nothing here opens the GPU."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fs():
    spec = importlib.util.spec_from_file_location("fs_keep_cpu", os.path.join(ROOT, "fusion_generation", "fusion_sampling.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


# ------------------------------------------------------------------------------------------------ --reroll
def test_reroll_parsing(fs):
    seg = "a cat+a dog+a tree"
    assert fs.parse_reroll("a dog", seg) == [1]
    assert fs.parse_reroll("2", seg) == [2]
    assert fs.parse_reroll("a tree+0", seg) == [0, 2]                       # phrases and indices mix; the result is sorted
    assert fs.parse_reroll(" a cat ", seg) == [0]
    for bad, word in (("a bird", "a bird"), ("3", "'3'"), ("-1", "-1"), ("", "''"), ("a cat+", "''"), ("1.0", "1.0")):
        with pytest.raises(SystemExit, match="--reroll") as e:
            fs.parse_reroll(bad, seg)
        assert word in str(e.value), (bad, str(e.value))
    for dup in ("a dog+a dog", "a dog+1", "0+0"):                            # the same region twice, however it is spelled
        with pytest.raises(SystemExit, match="twice"):
            fs.parse_reroll(dup, seg)
    with pytest.raises(SystemExit, match="--reroll"):
        fs.parse_reroll("0", "")                                            # no --seg_concepts: nothing to index


def test_keep_weight_from_masks(fs):
    """1 - min(1, sum of the re-rolled foreground masks), on the latent grid, from build_masks' own output"""
    from tweediemix_amd import masks as M
    H = W = 64
    a, b, c = (np.zeros((H, W), np.uint8) for _ in range(3))
    a[0:32, 0:32] = 255
    b[16:48, 16:48] = 255                                                    # overlaps a on [16,32) x [16,32)
    c[48:64, 48:64] = 255
    masks = M.build_masks([a, b, c], 8, 8, "cpu")
    assert masks.shape == (4, 1, 8, 8)
    one = fs.keep_weight(masks, [1])
    assert one.shape == (1, 1, 8, 8) and one.dtype == torch.float32 and one.is_contiguous()
    assert torch.equal(one, 1 - masks[1:2])
    both = fs.keep_weight(masks, [0, 1])                                     # two overlapping regions: the overlap counts once
    want = torch.ones(1, 1, 8, 8)
    want[..., 0:4, 0:4] = 0
    want[..., 2:6, 2:6] = 0
    assert torch.equal(both, want) and float(both.min()) == 0.0
    assert float((masks[0] + masks[1]).max()) == 2.0                         # (the sum itself does reach 2 there)
    assert torch.equal(fs.keep_weight(masks, [0, 1, 2]), 1 - masks[:3].sum(0, keepdim=True).clamp(max=1))
    assert set(torch.unique(both).tolist()) == {0.0, 1.0}


def test_keep_noise_is_the_second_draw_of_the_seed(fs):
    g = torch.Generator().manual_seed(41)
    x_t, second = torch.randn(1, 4, 16, 16, generator=g), torch.randn(1, 4, 16, 16, generator=g)
    assert torch.equal(fs.noise_for_seed(41, 16, 16), x_t)                   # a seed's x_T stays what it is
    assert torch.equal(fs.keep_noise_for_seed(41, 16, 16), second) and not torch.equal(second, x_t)


# ------------------------------------------------------------------------------------------------ refusals
BASE = ["--synthetic", "--tiny", "--concepts", "a+b+bg", "--seg_concepts", "a cat+a dog", "--resolution_h", "128", "--resolution_w", "128"]


def _files(tmp_path):
    from PIL import Image
    m = np.zeros((128, 128), np.uint8)
    m[:, :64] = 255
    Image.fromarray(m).save(tmp_path / "a cat.png")
    Image.fromarray(255 - m).save(tmp_path / "a dog.png")
    torch.save(torch.zeros(1, 4, 16, 16), tmp_path / "ok.latent.pt")
    torch.save(torch.zeros(1, 4, 32, 32), tmp_path / "big.latent.pt")
    torch.save({"x": 1}, tmp_path / "dict.latent.pt")
    Image.fromarray(np.zeros((128, 128, 3), np.uint8)).save(tmp_path / "ok.png")
    Image.fromarray(np.zeros((128, 96, 3), np.uint8)).save(tmp_path / "narrow.png")        # 96 wide, 128 high
    return f"{tmp_path / 'a cat.png'}+{tmp_path / 'a dog.png'}"


def test_every_refusal_is_a_system_exit_before_the_gpu(fs, tmp_path, monkeypatch):
    masks = _files(tmp_path)
    lat, img = str(tmp_path / "ok.latent.pt"), str(tmp_path / "ok.png")
    cases = [
        (["--reroll", "1"], "needs --keep_latents or --keep_image"),
        (["--keep_latents", lat, "--keep_image", img, "--mask_paths", masks, "--reroll", "1"], "mutually exclusive"),
        (["--keep_latents", lat, "--reroll", "1"], "--keep_latents needs --mask_paths"),
        (["--keep_image", img, "--reroll", "1"], "--keep_image needs --mask_paths"),
        (["--keep_latents", lat, "--reroll", "1", "--random_masks"], "needs --mask_paths"),
        (["--keep_latents", lat, "--reroll", "1", "--mask_source", "attention", "--mask_token_ids", "4+7"], "needs --mask_paths"),
        (["--keep_latents", lat, "--mask_paths", masks], "--keep_latents needs --reroll"),
        (["--keep_image", img, "--mask_paths", masks], "--keep_image needs --reroll"),
        (["--keep_latents", lat, "--mask_paths", masks, "--reroll", "a bird"], "a bird"),
        (["--keep_latents", lat, "--mask_paths", masks.split("+")[0], "--reroll", "1"], "has no mask"),
        (["--keep_latents", str(tmp_path / "missing.pt"), "--mask_paths", masks, "--reroll", "1"], "no such file"),
        (["--keep_latents", str(tmp_path / "big.latent.pt"), "--mask_paths", masks, "--reroll", "1"], r"\[1, 4, 16, 16\]"),
        (["--keep_latents", str(tmp_path / "dict.latent.pt"), "--mask_paths", masks, "--reroll", "1"], r"\[1, 4, 16, 16\]"),
        (["--keep_image", str(tmp_path / "narrow.png"), "--mask_paths", masks, "--reroll", "1"], "96 x 128"),
        (["--keep_image", str(tmp_path / "missing.png"), "--mask_paths", masks, "--reroll", "1"], "no such file"),
    ]

    def no_gpu(*a, **k):
        raise AssertionError("the GPU was touched before the refusal")
    for name in ("init", "_lazy_init", "set_device", "current_stream"):
        monkeypatch.setattr(torch.cuda, name, no_gpu)
    for extra, msg in cases:
        with pytest.raises(SystemExit, match=msg):
            fs.main(BASE + extra)
    # --keep_image without any VAE to encode it with (a real-weights run: no --vae_path, no vae/ under --sd_path)
    opt = fs.build_parser().parse_args(["--keep_image", img, "--mask_paths", masks, "--reroll", "1", "--seg_concepts", "a cat+a dog",
                                        "--resolution_h", "128", "--resolution_w", "128"])
    with pytest.raises(SystemExit, match="VAE encoder"):
        fs.check_keep_args(opt)
    # what is NOT refused: the checks hand back the parsed request, and a run without the flags has none
    opt = fs.build_parser().parse_args(BASE + ["--keep_latents", lat, "--mask_paths", masks, "--reroll", "a dog"])
    keep = fs.check_keep_args(opt)
    assert keep["reroll"] == [1] and tuple(keep["latent"].shape) == (1, 4, 16, 16) and keep["image"] is None
    opt = fs.build_parser().parse_args(BASE + ["--keep_image", img, "--mask_paths", masks, "--reroll", "0+1"])
    keep = fs.check_keep_args(opt)
    assert keep["reroll"] == [0, 1] and keep["latent"] is None and keep["image"].size == (128, 128) and keep["image"].mode == "RGB"
    assert fs.check_keep_args(fs.build_parser().parse_args(BASE)) is None


def test_new_flags_default_to_off(fs):
    opt = fs.build_parser().parse_args([])
    assert opt.keep_latents == "" and opt.keep_image == "" and opt.reroll == ""


# ------------------------------------------------------------------------------------------------ ABI
_CTYPE = {"const float*": C.c_void_p, "const void*": C.c_void_p, "float*": C.c_void_p, "void*": C.c_void_p, "int": C.c_int, "int64_t": C.c_int64}


def _prototype(name):
    src = open(os.path.join(ROOT, "include", "tmix.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", src, flags=re.S)
    assert m, f"{name} is not declared in include/tmix.h"
    return [re.sub(r"\s+", " ", a.strip()).rsplit(" ", 1) for a in m.group(1).split(",")]


def test_keep_prototype_matches_its_ctypes_declaration():
    from tweediemix_amd import lib
    new, old = _prototype("tmix_fused_tweedie_step_keep_dev"), _prototype("tmix_fused_tweedie_step_dev")
    # everything tmix_fused_tweedie_step_dev takes, same order, then the three keep arrays with their seed strides, then the stream
    assert new[:len(old) - 1] == old[:-1] and new[-1] == old[-1] == ["void*", "stream"]
    assert new[len(old) - 1:-1] == [["const float*", "keep_x0"], ["int64_t", "keep_x0_seed_stride"], ["const float*", "keep_eps"],
                                    ["int64_t", "keep_eps_seed_stride"], ["const float*", "keep_w"], ["int64_t", "keep_w_seed_stride"]]
    res, args = lib.SIGNATURES["tmix_fused_tweedie_step_keep_dev"]
    assert res is C.c_int and args == [_CTYPE[t] for t, _n in new]
    assert lib.SIGNATURES["tmix_fused_tweedie_step_dev"][1] == [_CTYPE[t] for t, _n in old]
    l = lib.load()
    assert l.tmix_fused_tweedie_step_keep_dev.argtypes == args and l.tmix_version() == 100


def test_keep_entry_validates_before_any_launch():
    """the error codes of the entry, seen without a GPU: validation comes first, nothing is dereferenced or launched"""
    from tweediemix_amd import lib
    l = lib.load()
    f = 0x1000
    K, hw, n = 3, 64, 256
    ok = dict(x=f, eps=f, dt=0, masks=f, mss=0, out=f, out0=None, K=K, ch=4, hw=hw, mode=lib.STEP_FUSION, rows=K + 1, seeds=2, prm=f,
              kx=f, sx=0, ke=f, se=n, kw=f, sw=0)

    def rc(**kw):
        a = dict(ok, **kw)
        return l.tmix_fused_tweedie_step_keep_dev(*[a[k] for k in ok], None)
    for name in ("kx", "ke", "kw"):
        assert rc(**{name: None}) == lib.EINVAL and b"keep pointer" in l.tmix_last_error_string(), name
    for name, short in (("sx", n - 1), ("se", n - 1), ("sw", hw - 1), ("sx", 1), ("sw", -hw)):
        assert rc(**{name: short}) == lib.ESHAPE and b"stride" in l.tmix_last_error_string(), (name, short)
    # the checks it shares with tmix_fused_tweedie_step_dev
    assert rc(x=None) == lib.EINVAL and rc(prm=None) == lib.EINVAL and rc(masks=None) == lib.EINVAL and rc(mode=3) == lib.EINVAL
    assert rc(rows=K) == lib.ESHAPE and rc(seeds=0) == lib.ESHAPE and rc(hw=0) == lib.ESHAPE and rc(dt=7) == lib.EINVAL
