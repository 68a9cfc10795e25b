"""CPU: the batched video path's host side -- the new C symbols, run_video.py's video list / sharding / padding / output names,
the refusal of --conditioning_path for several videos, and a world-2 gloo gather of video latents [n, 4, F, h, w]."""
import ctypes as C
import importlib.util
import os
import re
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tmix_video_step_prologue", "tmix_vpred_step_dev")


def _cli():
    spec = importlib.util.spec_from_file_location("run_video_batch_cli", os.path.join(ROOT, "run_video.py"))
    rv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rv)
    return rv


def test_new_symbols_declared_exported_and_typed():
    from tweediemix_amd import lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tmix.h")).read(), flags=re.S)
    l = lib.load()
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", src), name
        assert name in lib.SIGNATURES and hasattr(l, name)
    assert len(lib.SIGNATURES["tmix_video_step_prologue"][1]) == 14
    assert len(lib.SIGNATURES["tmix_vpred_step_dev"][1]) == 11


def test_new_entry_points_validate_before_launch():
    """null pointers -> TMIX_EINVAL, empty shapes / short clip strides -> TMIX_ESHAPE (checked before any launch: no GPU needed)."""
    from tweediemix_amd import lib as L
    l = L.load()
    p = C.c_void_p(64)                      # never dereferenced: every call below fails validation
    S, Cc, F, hw, R = 2, 4, 16, 64, 8
    clip_in, clip_out = F * R * hw, F * Cc * hw
    assert l.tmix_video_step_prologue(None, p, clip_in, p, p, clip_in, p, p, S, Cc, F, hw, R, None) == L.EINVAL
    assert l.tmix_video_step_prologue(p, p, clip_in, p, p, clip_in, p, None, S, Cc, F, hw, R, None) == L.EINVAL
    assert l.tmix_video_step_prologue(p, p, clip_in, p, p, clip_in, p, p, 0, Cc, F, hw, R, None) == L.ESHAPE
    assert l.tmix_video_step_prologue(p, p, clip_in, p, p, clip_in, p, p, S, Cc, F, hw, Cc - 1, None) == L.ESHAPE
    assert l.tmix_video_step_prologue(p, p, clip_in - 1, p, p, clip_in, p, p, S, Cc, F, hw, R, None) == L.ESHAPE
    assert l.tmix_vpred_step_dev(None, p, clip_out, p, clip_out, p, S, Cc, F, hw, None) == L.EINVAL
    assert l.tmix_vpred_step_dev(p, p, clip_out, None, clip_out, p, S, Cc, F, hw, None) == L.EINVAL
    assert l.tmix_vpred_step_dev(p, p, clip_out, p, clip_out, p, S, Cc, 0, hw, None) == L.ESHAPE
    assert l.tmix_vpred_step_dev(p, p, clip_out, p, clip_out - 1, p, S, Cc, F, hw, None) == L.ESHAPE
    assert b"clip stride" in l.tmix_last_error_string()


def test_video_list_is_images_by_seeds_image_major():
    rv = _cli()
    assert rv.video_list(["a.png", "b.png"], 7, 3) == [("a.png", 7), ("a.png", 8), ("a.png", 9), ("b.png", 7), ("b.png", 8), ("b.png", 9)]
    opt = rv.build_parser().parse_args(["--image_path", "x/a.png+y/b.png", "--num_seeds", "2", "--seed", "5"])
    images, videos = rv.check_args(opt)
    assert images == ["x/a.png", "y/b.png"] and videos == [("x/a.png", 5), ("x/a.png", 6), ("y/b.png", 5), ("y/b.png", 6)]
    opt = rv.build_parser().parse_args([])
    assert rv.check_args(opt)[1] == [(opt.image_path, 6425)]          # the default invocation is one video


def test_round_robin_sharding_of_videos():
    from tweediemix_amd import dist as D
    rv = _cli()
    videos = rv.video_list(["a", "b"], 0, 3)
    shards = [D.seed_shard(videos, r, 4) for r in range(4)]
    assert shards[0] == [("a", 0), ("b", 1)] and shards[1] == [("a", 1), ("b", 2)] and shards[2] == [("a", 2)] and shards[3] == [("b", 0)]
    assert sorted(v for s in shards for v in s) == sorted(videos)


def test_ragged_batch_is_padded_then_trimmed():
    rv = _cli()
    assert rv.padded_batches([0, 1, 2], 2) == [([0, 1], 2), ([2, 2], 1)]
    assert rv.padded_batches([0, 1, 2, 3, 4], 4) == [([0, 1, 2, 3], 4), ([4, 4, 4, 4], 1)]
    assert rv.padded_batches(list(range(6)), 3) == [([0, 1, 2], 3), ([3, 4, 5], 3)]
    assert rv.padded_batches([], 4) == []


def test_output_names_for_one_and_several_images():
    rv = _cli()
    assert rv.output_stem("dir/cat dog.png", 6425, False) == "output_i2v_seed_6425"
    assert rv.output_stem("dir/cat dog.png", 6425, True) == "cat dog_seed_6425"
    assert rv.output_stem("b.jpeg", 3, True) == "b_seed_3"


@pytest.mark.parametrize("extra", [["--num_seeds", "2"], ["--image_path", "a.png+b.png"]])
def test_conditioning_path_refused_for_several_videos(extra, tmp_path, monkeypatch):
    rv = _cli()
    monkeypatch.chdir(tmp_path)
    with pytest.raises(SystemExit) as e:
        rv.main(["--synthetic", "--tiny", "--conditioning_path", "c.pt"] + extra)
    assert "--conditioning_path" in str(e.value) and "ONE video" in str(e.value)
    assert not any(tmp_path.iterdir())                                 # refused before anything ran


@pytest.mark.parametrize("bad", [["--gpus", "9"], ["--gpus", "0"], ["--num_seeds", "0"]])
def test_bad_counts_refused(bad):
    rv = _cli()
    with pytest.raises(SystemExit):
        rv.main(["--synthetic", "--tiny"] + bad)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from tweediemix_amd import dist as D
    spec = importlib.util.spec_from_file_location("run_video_batch_cli_w", os.path.join(ROOT, "run_video.py"))
    rv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rv)
    videos = rv.video_list(["a", "b"], 10, 3)                          # 6 videos, 3 per rank
    mine = D.seed_shard(videos, rank, world)
    F, h, w = 16, 3, 5
    lat = lambda v: torch.full((4, F, h, w), float(v[1] + (100 if v[0] == "b" else 0))) + torch.arange(float(F))[:, None, None]
    local = torch.stack([lat(v) for v in mine])
    allx = D.gather_latents(local, len(videos), rank, world)
    q.put((rank, tuple(allx.shape), all(torch.equal(allx[i], lat(v)) for i, v in enumerate(videos))))
    dist.barrier()
    dist.destroy_process_group()


def test_gather_of_video_latents_world2():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert all(shape == (6, 4, 16, 3, 5) and ok for _r, shape, ok in res), res
