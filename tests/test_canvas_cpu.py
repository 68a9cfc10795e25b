"""CPU: the wide canvas without a GPU -- the window layout rule (tweediemix_amd/canvas.py), the ctypes declaration of tmix_window_consensus against
its prototype in include/tmix.h, its argument errors (all reported on the host before any launch), and the command-line half
(--canvas_h / --canvas_w / --window_overlap of fusion_generation/fusion_sampling.py).  Nothing here opens the GPU."""
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
    spec = importlib.util.spec_from_file_location("fs_canvas_cpu", os.path.join(ROOT, "fusion_generation", "fusion_sampling.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


# ------------------------------------------------------------------------------------------------ layout
def test_layout_rule_table():
    from tweediemix_amd import canvas as CV
    assert CV.axis_offsets(40, 16, 4) == [0, 12, 24]
    assert CV.axis_offsets(28, 16, 12) == [0, 4, 8, 12]
    assert CV.axis_offsets(72, 16, 8) == [0, 8, 16, 24, 32, 40, 48, 56]
    assert CV.axis_offsets(256, 128, 64) == [0, 64, 128]
    assert CV.axis_offsets(17, 16, 8) == [0, 1]
    assert CV.axis_offsets(16, 16, 8) == [0] and CV.axis_offsets(16, 16, 0) == [0]
    # 192 x 256 canvas, 128 windows, overlap 64: 2 x 3 windows, row-major with y outer
    assert CV.window_layout(192, 256, 128, 128, 64) == [(0, 0), (0, 64), (0, 128), (64, 0), (64, 64), (64, 128)]
    cover = np.zeros(28, int)                                   # 28 / 16 / 12: up to four windows cover a pixel
    for o in CV.axis_offsets(28, 16, 12):
        cover[o:o + 16] += 1
    assert cover.max() == 4 and cover[0] == cover[-1] == 1
    for bad in ((15, 16, 4), (40, 16, 16), (40, 16, -1), (40, 0, 0)):
        with pytest.raises(ValueError, match="window layout"):
            CV.axis_offsets(*bad)


def test_layout_rule_random_cases():
    """every canvas pixel covered, the edge pixels exactly once, the first window at 0 and the last flush with the far edge (so (n - 1) divides
    (n - 1) * (c - s) exactly there), neighbours overlapping by at least o, the window count the rule's"""
    from tweediemix_amd import canvas as CV
    rng = np.random.RandomState(0)
    for _ in range(500):
        s = int(rng.randint(1, 40))
        o = int(rng.randint(0, s))
        c = s + int(rng.randint(0, 200))
        offs = CV.axis_offsets(c, s, o)
        n = len(offs)
        cover = np.zeros(c, int)
        for off in offs:
            assert 0 <= off <= c - s
            cover[off:off + s] += 1
        assert cover.min() >= 1 and cover[0] == 1 and cover[-1] == 1, (c, s, o)
        assert offs[0] == 0 and offs[-1] == c - s and offs == sorted(set(offs)), (c, s, o)
        if c == s:
            assert n == 1
            continue
        assert n == -((c - o) // -(s - o)) and ((n - 1) * (c - s)) % (n - 1) == 0
        assert all(b - a <= s - o for a, b in zip(offs, offs[1:])), (c, s, o, offs)


def test_tent_crop_assemble():
    from tweediemix_amd import canvas as CV
    t = CV.tent_weight(5, 8)
    assert t.dtype == torch.float32 and t.shape == (5, 8)
    assert t[:, 0].tolist() == [1, 2, 3, 2, 1] and t[0].tolist() == [1, 2, 3, 4, 4, 3, 2, 1] and float(t[2, 3]) == 12
    offs = CV.window_layout(24, 24, 16, 16, 8)
    assert offs == [(0, 0), (0, 8), (8, 0), (8, 8)]
    canvas = torch.arange(2 * 3 * 24 * 24, dtype=torch.float32).reshape(2, 3, 24, 24)
    wins = CV.crop_windows(canvas, offs, 16, 16)
    assert wins.shape == (8, 3, 16, 16) and wins.is_contiguous()
    assert torch.equal(wins[5], canvas[1, :, 0:16, 8:24])                     # group-major: b = group * n_win + window
    assert torch.equal(CV.assemble(wins, offs, 24, 24), canvas)


# ------------------------------------------------------------------------------------------------ ABI
_CTYPE = {"const float*": C.c_void_p, "float*": C.c_void_p, "void*": C.c_void_p, "int": C.c_int, "int64_t": C.c_int64,
          "const int*": C.POINTER(C.c_int32)}


def _prototype(name):
    src = open(os.path.join(ROOT, "include", "tmix.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", src, flags=re.S)
    assert m, f"{name} is not declared in include/tmix.h"
    return [re.sub(r"\s+", " ", a.strip()).rsplit(" ", 1) for a in m.group(1).split(",")]


def test_consensus_prototype_matches_its_ctypes_declaration():
    from tweediemix_amd import lib
    proto = _prototype("tmix_window_consensus")
    assert proto == [["float*", "x"], ["int", "groups"], ["int", "n_win"], ["const int*", "win_yx"], ["int", "C"], ["int", "h"], ["int", "w"],
                     ["int", "canvas_h"], ["int", "canvas_w"], ["const float*", "weight"], ["void*", "stream"]]
    res, args = lib.SIGNATURES["tmix_window_consensus"]
    assert res is C.c_int and args == [_CTYPE[t] for t, _n in proto]
    l = lib.load()
    assert l.tmix_window_consensus.argtypes == args and l.tmix_version() == 100
    src = open(os.path.join(ROOT, "include", "tmix.h")).read()
    assert re.search(r"#define\s+TMIX_MAX_WINDOWS\s+8\b", src) and lib.MAX_WINDOWS == 8


def test_consensus_entry_validates_before_any_launch():
    """every argument error of the entry, seen without a GPU: validation comes first, nothing is dereferenced or launched"""
    from tweediemix_amd import lib
    l = lib.load()
    f = 0x1000
    ok = dict(x=f, groups=2, n_win=3, yx=[0, 0, 0, 12, 0, 24], C=4, h=16, w=16, ch=16, cw=40, weight=None)

    def rc(**kw):
        a = dict(ok, **kw)
        yx = None if a["yx"] is None else (C.c_int32 * len(a["yx"]))(*a["yx"])
        return l.tmix_window_consensus(a["x"], a["groups"], a["n_win"], yx, a["C"], a["h"], a["w"], a["ch"], a["cw"], a["weight"], None)

    def err():
        return l.tmix_last_error_string()
    assert rc(x=None) == lib.EINVAL and b"null" in err()
    assert rc(yx=None) == lib.EINVAL and b"null" in err()
    eight = [v for i in range(8) for v in (0, 8 * i)]
    for n_win, yx in ((0, ok["yx"]), (-1, ok["yx"]), (9, eight + [0, 56])):
        assert rc(n_win=n_win, yx=yx, cw=72) == lib.EINVAL and b"n_win" in err(), n_win
    for groups in (0, -3):
        assert rc(groups=groups) == lib.EINVAL and b"groups" in err()
    # a window that reaches outside the canvas: behind the right / bottom edge, a negative corner, a canvas smaller than the window
    for bad in (dict(yx=[0, 0, 0, 12, 0, 25]), dict(yx=[0, 0, 0, 12, 1, 24]), dict(yx=[0, -1, 0, 12, 0, 24]), dict(yx=[-1, 0, 0, 12, 0, 24]),
                dict(cw=39), dict(ch=15), dict(yx=[0, 0, 0, 12, 0, 2 ** 31 - 8])):
        assert rc(**bad) == lib.ESHAPE and b"outside" in err(), bad
    # a canvas pixel that no window covers: a gap between windows, an uncovered edge column / row, an uncovered corner of a 2 x 2 layout
    for bad in (dict(yx=[0, 0, 0, 4, 0, 24]), dict(cw=41), dict(ch=17), dict(yx=[0, 1, 0, 12, 0, 24]),
                dict(yx=[0, 0, 0, 8, 8, 0], ch=24, cw=24)):
        assert rc(**bad) == lib.ESHAPE and b"uncovered" in err(), bad
    for bad in (dict(C=0), dict(h=0), dict(w=-16), dict(ch=0), dict(cw=0), dict(C=-4)):
        assert rc(**bad) == lib.ESHAPE and b"non-positive" in err(), bad
    # what is NOT refused, still without a launch: one window that is the canvas (nothing to reconcile)
    assert rc(n_win=1, yx=[0, 0], cw=16) == 0
    assert rc(n_win=1, yx=[0, 0], cw=16, groups=7, C=3, h=5, w=7, ch=5) == lib.ESHAPE            # (one 5 x 7 window is not a 5 x 16 canvas)
    assert rc(n_win=1, yx=[0, 0], groups=7, C=3, h=5, w=7, ch=5, cw=7) == 0


def test_ops_wrapper_refuses_cpu_tensors():
    from tweediemix_amd import lib, ops
    with pytest.raises(lib.TmixError):
        ops.window_consensus(torch.zeros(3, 4, 16, 16), 1, [(0, 0), (0, 12), (0, 24)], (16, 40))


# ------------------------------------------------------------------------------------------------ CLI
BASE = ["--synthetic", "--tiny", "--concepts", "a+b+bg", "--seg_concepts", "a cat+a dog", "--resolution_h", "128", "--resolution_w", "128"]


def test_cli_refusals_come_before_the_gpu(fs, tmp_path, monkeypatch):
    torch.save(torch.zeros(1, 4, 16, 16), tmp_path / "ok.latent.pt")
    lat = str(tmp_path / "ok.latent.pt")
    wide = ["--canvas_w", "320"]
    cases = [
        (wide + ["--keep_latents", lat, "--mask_paths", "a.png+b.png", "--reroll", "1"], "--keep_latents"),
        (wide + ["--keep_image", "x.png", "--mask_paths", "a.png+b.png", "--reroll", "1"], "--keep_image"),
        (wide + ["--reroll", "1"], "--reroll"),
        (wide + ["--mask_source", "attention", "--mask_token_ids", "4+7"], "--mask_source attention"),
        (wide + ["--streams", "2"], "--streams 2"),
        (["--canvas_w", "324"], "multiples of 8"),
        (["--canvas_h", "132"], "multiples of 8"),
        (["--canvas_w", "120"], "smaller than the window"),
        (["--canvas_h", "64", "--canvas_w", "320"], "smaller than the window"),
        (wide + ["--window_overlap", "128"], "--window_overlap 128"),
        (wide + ["--window_overlap", "136"], "--window_overlap 136"),
        (wide + ["--window_overlap", "30"], "--window_overlap 30"),
        (["--window_overlap", "32"], "--window_overlap"),
        (["--canvas_w", "1024", "--window_overlap", "0"], "8 windows"),                                  # at most 8: 1024 / 128 = 8 fit ...
        (["--canvas_w", "1032", "--window_overlap", "0"], "9 windows"),                                  # ... a ninth does not
        (["--canvas_h", "256", "--canvas_w", "384", "--window_overlap", "64"], "15 windows"),            # 3 x 5
        (wide + ["--window_overlap", "32", "--num_seeds", "3", "--seeds_per_batch", "3"], "9 co-batched"),
    ]

    def no_gpu(*a, **k):
        raise AssertionError("the GPU was touched before the refusal")
    for name in ("init", "_lazy_init", "set_device", "current_stream"):
        monkeypatch.setattr(torch.cuda, name, no_gpu)
    for extra, msg in cases:
        if msg == "8 windows":                       # (exactly 8 windows is allowed: checked below, not a refusal)
            continue
        with pytest.raises(SystemExit, match=msg):
            fs.main(BASE + extra)
    parse = lambda extra: fs.check_canvas_args(fs.build_parser().parse_args(BASE + extra))
    assert parse([]) is None
    assert parse(["--canvas_w", "128"]) is None and parse(["--canvas_h", "128", "--canvas_w", "128", "--window_overlap", "32"]) is None
    assert parse(wide) == dict(height=128, width=320, overlap=64, n_win=4)               # default overlap: half the smaller window side
    assert parse(wide + ["--window_overlap", "32"]) == dict(height=128, width=320, overlap=32, n_win=3)
    assert parse(["--canvas_w", "1024", "--window_overlap", "0"])["n_win"] == 8
    assert parse(["--canvas_h", "192", "--canvas_w", "256"]) == dict(height=192, width=256, overlap=64, n_win=6)
    # --mask_paths / --random_masks win over --mask_source attention, with a canvas too
    assert parse(wide + ["--mask_source", "attention", "--random_masks"])["n_win"] == 4


def test_new_flags_default_to_off(fs):
    opt = fs.build_parser().parse_args([])
    assert opt.canvas_h == 0 and opt.canvas_w == 0 and opt.window_overlap == -1
    assert fs.check_canvas_args(opt) is None


def test_default_seeds_per_batch(fs):
    # without a canvas: what it always was (all seeds of the rank, at most 4)
    assert [fs.default_seeds_per_batch(n) for n in (0, 1, 3, 4, 9)] == [1, 1, 3, 4, 4]
    # with a canvas: seeds x windows stays within the 8 co-batched row sets
    assert [fs.default_seeds_per_batch(n, 3) for n in (0, 1, 2, 5)] == [1, 1, 2, 2]
    assert [fs.default_seeds_per_batch(n, 2) for n in (1, 4, 9)] == [1, 4, 4]
    assert fs.default_seeds_per_batch(5, 4) == 2 and fs.default_seeds_per_batch(5, 6) == 1 and fs.default_seeds_per_batch(5, 8) == 1


def test_sampler_limits_name_the_numbers():
    """Tweediemix(canvas=...) refuses what it cannot do with a ValueError, before it builds a plan (a CPU stand-in for the weights is enough)"""
    from tweediemix_amd import sampler as S

    class NoWeights:
        device = torch.device("cpu")
        kind = "custom"
    cfg = S.make_config(n_timesteps=10, resolution_h=128, resolution_w=128, jumping_steps=1)
    mk = lambda **kw: S.Tweediemix(cfg, NoWeights(), None, None, None, concept_num=3, **kw)
    wide = dict(height=128, width=320, overlap=32)                            # three windows
    with pytest.raises(ValueError, match=r"3 windows x 3 seeds = 9"):
        mk(canvas=wide, n_seeds=3)
    with pytest.raises(ValueError, match="attention_masks"):
        mk(canvas=wide, attention_masks=dict(tokens=[[4], [7]]))
    with pytest.raises(ValueError, match="n_streams = 2"):
        mk(canvas=wide, n_streams=2)
    with pytest.raises(ValueError, match="multiples of 8"):
        mk(canvas=dict(height=128, width=324, overlap=32))
    with pytest.raises(ValueError, match="overlap"):
        mk(canvas=dict(height=128, width=320, overlap=128))
    with pytest.raises(ValueError, match="must hold"):
        mk(canvas=dict(height=64, width=320, overlap=32))
    tw = mk(canvas=wide, n_seeds=2)
    assert tw.windows == [(0, 0), (0, 12), (0, 24)] and tw.n_seeds == 6 and tw.n_canvas == 2 and (tw.canvas_h, tw.canvas_w) == (16, 40)
    assert tuple(tw.x_state.shape) == (6, 4, 16, 16)
    z = torch.zeros(2, 4, 16, 16)
    with pytest.raises(ValueError, match="set_keep"):
        tw.set_keep(z[:1], z[:1, :1], z)
    # a canvas of the window's size is no canvas: one window, the sampler of today (set_keep included)
    one = mk(canvas=dict(height=128, width=128, overlap=64), n_seeds=2, n_streams=2)
    assert one.windows is None and one.n_seeds == 2 and tuple(one.x_state.shape) == (2, 4, 16, 16)
    one.set_keep(z[:1], z[:1, :1], z)
