"""CPU: the guidance interval on the host -- the numpy restatement of tmix_fused_tweedie_step_cond_dev against hand-computed elements,
the parsing and every refusal (raised before any device use), which schedule entries are unguided on the 'leading' and the 'logsnr' grid, the
order rule of the solver at both borders of the interval, and the defaults: a full interval changes nothing.  No test here launches anything: the
samplers live on the CPU device with their step replaced by a recorder."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import guidance_interval_cases as GC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NF = np.float32


# ------------------------------------------------------------------------------------------------ the restatement
def test_restatement_against_hand_computed_elements():
    """every value is a dyadic rational, so each operation is exact and the expected numbers are plain arithmetic:
    sa = 0.5, s1 = 0.25, x = 2, rows e = (4, -8, 0), masks m = (0.5, 0.25, 0.25):
      t_c = (2 - 0.25 e_c) / 0.5 = (2, 8, 4);  FUSION x0 = 0.5*2 + 0.25*8 + 0.25*4 = 4;  PLAIN x0 = t_0 = 2
      DDIM (sa' = 0.75, s1' = 0.5): e0 = (2 - 0.5 x0) / 0.25 -> FUSION 0, PLAIN 4;  moved = 0.75 x0 + 0.5 e0 -> FUSION 3, PLAIN 3.5
      multistep (cx = 0.5, c0 = 0.25, c1 = -0.125, x0_prev = 8): moved = 0.5*2 + (0.25 x0 - 1) -> FUSION 1, PLAIN 0.5; first order: 2 and 1.5"""
    from tweediemix_amd import guidance as G
    x = np.full((1, 1, 1, 2), 2.0, NF)
    eps = np.stack([np.full((1, 1, 2), v, NF) for v in (4.0, -8.0, 0.0)])
    masks = np.stack([np.full((1, 1, 2), v, NF) for v in (0.5, 0.25, 0.25)])
    prev = np.full_like(x, 8.0)
    ddim = [500.0, 0.5, 0.25, 0.75, 0.5, 0.0, 123.0, 0.0]                     # the g slot (123) is ignored
    for mode, x0, moved in ((GC.STEP_FUSION, 4.0, 3.0), (GC.STEP_PLAIN, 2.0, 3.5)):
        out, e0 = G.cond_step_reference(mode, x, eps, masks, None, ddim)
        assert out.dtype == NF and np.all(out == moved) and np.all(e0 == x0), (mode, out, e0)
        out, e0 = G.cond_step_reference(mode, x, eps, masks, None, ddim[:5] + [1.0, 0.0, 0.0])           # is_last: x0 itself
        assert np.all(out == x0) and np.all(e0 == x0)
    for mode, x0, second, first in ((GC.STEP_FUSION, 4.0, 1.0, 2.0), (GC.STEP_PLAIN, 2.0, 0.5, 1.5)):
        out, e0 = G.cond_step_reference(mode, x, eps, masks, prev, [500.0, 0.5, 0.25, 0.5, 0.25, -0.125, 0.0, 123.0])
        assert np.all(out == second) and np.all(e0 == x0)
        nan_prev = np.full_like(x, np.nan)                                     # a first-order step does not read the history
        out, e0 = G.cond_step_reference(mode, x, eps, masks, nan_prev, [500.0, 0.5, 0.25, 0.5, 0.25, 0.0, 0.0, 123.0])
        assert np.all(out == first) and np.all(e0 == x0)
        out, _ = G.cond_step_reference(mode, x, eps, masks, prev, [500.0, 0.5, 0.25, 0.5, 0.25, -0.125, 1.0, 123.0])
        assert np.all(out == x0)
    # s1 == 0 (alpha = 1): e0 is 0 by definition, moved = sa' x0
    out, e0 = G.cond_step_reference(GC.STEP_PLAIN, x, eps, None, None, [1.0, 1.0, 0.0, 0.75, 0.5, 0.0, 0.0, 0.0])
    assert np.all(e0 == 2.0) and np.all(out == 1.5)
    with pytest.raises(ValueError, match="FUSION or PLAIN"):
        G.cond_step_reference(GC.STEP_RESAMPLE, x, eps, masks, None, ddim)


def test_restatement_noise_and_fp16_rounding_points():
    """with a key the move gains one product and one sum, cz * z of noise.normal at the element's index and the params' step; the last step gains
    nothing.  fp16 eps: the products s1 * e_c and s1' * e0 round to fp16, nothing else does"""
    from tweediemix_amd import guidance as G, noise as NZ
    rng = np.random.RandomState(5)
    x = rng.randn(1, 4, 3, 5).astype(NF)
    eps = rng.randn(3, 4, 3, 5).astype(np.float16).astype(NF)
    masks = rng.rand(3, 1, 3, 5).astype(NF)
    key = NZ.seed_key(GC.SEEDS64[1])
    p8 = [float(NF(v)) for v in (612.0, 0.48, 0.877, 0.62, 0.78, 0.0, 9.0, 0.0)]
    base, x0 = G.cond_step_reference(GC.STEP_FUSION, x, eps, masks, None, p8)
    nz, x0n = G.cond_step_reference(GC.STEP_FUSION, x, eps, masks, None, p8 + [0.3125, 7.0, 0.0, 0.0], key)
    z = NZ.normal(np.arange(x.size, dtype=np.uint64).reshape(x.shape), key[0], key[1], 7)
    assert np.array_equal(x0, x0n) and np.array_equal(nz, (base + (NF(0.3125) * z).astype(NF)).astype(NF)) and not np.array_equal(nz, base)
    idx = NZ.canvas_index(4, 3, 5, 2, 1, 8, 9)
    nzc, _ = G.cond_step_reference(GC.STEP_FUSION, x, eps, masks, None, p8 + [0.3125, 7.0, 0.0, 0.0], key, idx)
    assert np.array_equal(nzc, (base + (NF(0.3125) * NZ.normal(idx, key[0], key[1], 7)).reshape(x.shape).astype(NF)).astype(NF))
    lastp = p8[:5] + [1.0, 9.0, 0.0, 0.3125, 7.0, 0.0, 0.0]
    out, _ = G.cond_step_reference(GC.STEP_FUSION, x, eps, masks, None, lastp, key)
    assert np.array_equal(out, x0)
    same, _ = G.cond_step_reference(GC.STEP_FUSION, x, eps, masks, None, p8 + [0.0, 7.0, 0.0, 0.0], key)       # cz == 0
    assert np.array_equal(same, base)
    # fp16: written out for the PLAIN form
    sa, s1, san, s1n = (NF(v) for v in p8[1:5])
    h = lambda a: a.astype(np.float16).astype(NF)
    t0 = ((x - h(s1 * eps[:1])) / sa).astype(NF)
    e0 = ((x - (sa * t0).astype(NF)) / s1).astype(NF)
    want = ((san * t0).astype(NF) + h((s1n * e0).astype(NF))).astype(NF)
    got, g0 = G.cond_step_reference(GC.STEP_PLAIN, x, eps, None, None, p8, lowp=np.float16)
    assert np.array_equal(g0, t0) and np.array_equal(got, want)
    assert not np.array_equal(got, G.cond_step_reference(GC.STEP_PLAIN, x, eps, None, None, p8)[0])


def test_unguided_x0_is_the_guided_x0_of_a_copied_row():
    """the parents' restatements with the unconditional row a copy of the conditional one (any finite g) give the same x0: cfg(e, e, g) = e"""
    from tweediemix_amd import guidance as G, solver as SV
    rng = np.random.RandomState(6)
    x, e = rng.randn(1, 4, 5, 7).astype(NF), rng.randn(1, 4, 5, 7).astype(NF)
    for g in (9.0, 0.8, -3.5):
        a = SV.blended_x0_reference(GC.STEP_PLAIN, x, np.concatenate([e, e]), None, g, NF(0.48), NF(0.877))
        assert np.array_equal(a, G.cond_x0_reference(GC.STEP_PLAIN, x, e, None, NF(0.48), NF(0.877)))


# ------------------------------------------------------------------------------------------------ parsing and refusals
def test_interval_parsing():
    from tweediemix_amd import guidance as G
    assert G.validate_interval(None) is None
    assert G.validate_interval("700,250") == (700, 250) and G.validate_interval(" 1000 , 0 ") == (1000, 0) and G.validate_interval("5,5") == (5, 5)
    assert G.validate_interval((700, 250)) == (700, 250) and G.validate_interval([np.int64(9), 3]) == (9, 3)
    for bad in ("", "700", "700,250,1", "250,700", "1001,0", "5,-1", "7.5,2", "a,b", "700;250", (700,), (250, 700), (700.0, 250), (True, 0), 700,
                (1001, 5), (5, -1)):
        with pytest.raises(ValueError, match="T_HI,T_LO"):
            G.validate_interval(bad)
    with pytest.raises(ValueError, match="--guidance_interval"):
        G.validate_interval("9", "--guidance_interval")
    assert G.is_guided(None, 999) and G.is_guided((700, 250), 700) and G.is_guided((700, 250), 250)
    assert not G.is_guided((700, 250), 701) and not G.is_guided((700, 250), 249)


class _Untouchable:
    """weights whose device must not even be asked for: the refusal comes first"""
    kind = "custom"

    @property
    def device(self):
        raise AssertionError("the device was touched before the refusal")


def test_sampler_refusals_come_before_any_device_use():
    from tweediemix_amd import sampler as S
    for bad in ("250,700", (250, 700), "x", (1001, 0)):
        with pytest.raises(ValueError, match="guidance_interval"):
            S.Tweediemix(GC.make_cfg(S), _Untouchable(), None, None, None, concept_num=3, guidance_interval=bad)
    tw, _ = GC.standin_sampler("cpu", guidance_interval=(700, 250))
    assert tw.guidance_interval == (700, 250)
    z = torch.zeros(1, 4, GC.H, GC.W)
    with pytest.raises(ValueError, match=r"set_keep: not with guidance_interval=\(700, 250\)"):
        tw.set_keep(z, z[:, :1], z)
    assert tw._keep is None
    tw, _ = GC.standin_sampler("cpu")                    # without an interval the keep region is set as before
    tw.set_keep(z, z[:, :1], z)
    assert tw._keep is not None and tw.guidance_interval is None


def _cli():
    spec = importlib.util.spec_from_file_location("fs_cli_interval", os.path.join(ROOT, "fusion_generation", "fusion_sampling.py"))
    fs = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fs)
    return fs


def test_cli_flag_and_refusals(tmp_path, monkeypatch):
    fs = _cli()
    opt = fs.build_parser().parse_args([])
    assert opt.guidance_interval == ""
    fs.check_solver_args(opt)
    assert opt.guidance_interval is None
    opt = fs.build_parser().parse_args(["--guidance_interval", "700,250"])
    fs.check_solver_args(opt)
    assert opt.guidance_interval == (700, 250)
    assert "T_HI,T_LO" in fs.build_parser().format_help()

    def no_gpu(*a, **k):
        raise AssertionError("the GPU was touched before the refusal")
    for name in ("init", "_lazy_init", "set_device", "current_stream"):
        monkeypatch.setattr(torch.cuda, name, no_gpu)
    common = ["--synthetic", "--tiny", "--concepts", "cat+dog+bg", "--seg_concepts", "a cat+a dog", "--prompt_orig", "p", "--output_path", str(tmp_path),
              "--resolution_h", "128", "--resolution_w", "128"]
    torch.save(torch.zeros(1, 4, 16, 16), tmp_path / "kept")
    keep = ["--mask_paths", "a.png+b.png", "--reroll", "1"]
    for bad in ("250,700", "700", "1001,0", "7.5,2", "700,250,3"):
        with pytest.raises(SystemExit, match="--guidance_interval"):
            fs.main(common + ["--guidance_interval", bad])
    from PIL import Image
    Image.fromarray(np.zeros((128, 128, 3), np.uint8)).save(tmp_path / "kept.png")
    for flag, name in (("--keep_latents", "kept"), ("--keep_image", "kept.png")):
        with pytest.raises(SystemExit, match=f"--guidance_interval 700,250 does not combine with {flag}"):
            fs.main(common + ["--guidance_interval", "700,250", flag, str(tmp_path / name)] + keep)


# ------------------------------------------------------------------------------------------------ which steps are unguided
def _recorded_run(**kw):
    """run_fusion on the CPU device with _run_step replaced by a recorder: -> [(kind, mode, t, ms coefficients or None)] in call order"""
    from tweediemix_amd import sampler as S
    cfg = kw.pop("cfg", None) or GC.make_cfg(S, n=kw.pop("n", 10))
    tw, _ = GC.standin_sampler("cpu", cfg=cfg, **kw)
    calls = []

    def run_step(kind, mode, t, at, at_next, is_last=False, ms=None, step_index=None):
        calls.append((kind, mode, int(t), ms))
        tw.unet_calls.append((kind, GC.ROWS[kind], int(t)))
    tw._run_step = run_step
    tw.run_fusion(torch.zeros(1, 4, GC.H, GC.W))
    return tw, calls


def test_classification_on_the_leading_grid():
    """n = 10, 'leading': timesteps 901, 801, ..., 1; interval (700, 250) guides 601 .. 301.  The first timestep (start phase, resampling round
    trips) and the look-ahead stay guided whatever the interval says; 801 (plain) and 701, 201, 101, 1 (fusion) run without the unconditional row"""
    tw, calls = _recorded_run(guidance_interval=GC.INTERVAL)
    assert tw.scheduler.timesteps == [901, 801, 701, 601, 501, 401, 301, 201, 101, 1]
    assert [(k, t) for k, _m, t, _ in calls] == [
        ("start", 901), ("plain", 801), ("start", 901),                # one resampling round trip and the step of the first timestep: guided
        ("plain_c", 801), ("plain", 701),                              # 801 > 700: unguided; then its look-ahead (t_cond_prev = 801) at 701: guided
        ("fusion_c", 701), ("fusion", 601), ("fusion", 501), ("fusion", 401), ("fusion", 301),
        ("fusion_c", 201), ("fusion_c", 101), ("fusion_c", 1)]
    assert tw.unet_calls == [(k, GC.ROWS[k], t) for k, _m, t, _ in calls]
    assert [r for k, r, _t in tw.unet_calls if k.endswith("_c")] == [1, 3, 3, 3, 3]
    # borders are inclusive: (601, 301) guides exactly the same entries, (600, 302) two fewer
    assert [c[:3] for c in _recorded_run(guidance_interval=(601, 301))[1]] == [c[:3] for c in calls]
    kinds = [k for k, *_ in _recorded_run(guidance_interval=(600, 302))[1]]
    assert kinds[5:] == ["fusion_c", "fusion_c", "fusion", "fusion", "fusion_c", "fusion_c", "fusion_c", "fusion_c"]
    # an interval below the schedule's first step behind the start: everything behind the first timestep is unguided, the first timestep is not
    kinds = [k for k, *_ in _recorded_run(guidance_interval=(0, 0))[1]]
    assert kinds == ["start", "plain", "start", "plain_c", "plain"] + ["fusion_c"] * 8


def test_classification_on_the_logsnr_grid_keeps_the_noise_range():
    """the interval is in timestep VALUES: on the log-SNR grid (901, 770, 612, 427, 243, 108, 39, 12, 4, 1) the same (700, 250) guides 612 and 427 --
    other indices than on the leading grid, the same noise range"""
    tw, calls = _recorded_run(guidance_interval=GC.INTERVAL, timestep_spacing="logsnr")
    assert tw.scheduler.timesteps == [901, 770, 612, 427, 243, 108, 39, 12, 4, 1]
    trajectory = [(k, t) for k, _m, t, _ in calls[3:] if (k, t) != ("plain", 612)]
    assert calls[4][0] == "plain" and calls[4][2] == 612                         # the look-ahead
    assert trajectory == [("plain_c", 770), ("fusion", 612), ("fusion", 427)] + [("fusion_c", t) for t in (243, 108, 39, 12, 4, 1)]


def test_lora_window_kinds():
    """the LoRA window (t_stop): fusion_base behind the window and plain behind t_stop get their unguided twins as well"""
    tw, _ = GC.standin_sampler("cpu", guidance_interval=(700, 450), lora=True)
    calls = []
    tw._run_step = lambda kind, mode, t, *a, **k: calls.append((kind, int(t)))
    tw.run_fusion(torch.zeros(1, 4, GC.H, GC.W))
    traj = [c for i, c in enumerate(calls) if i >= 3 and c != ("plain", 701)]
    assert traj == [("plain_c", 801), ("fusion_c", 701), ("fusion", 601), ("fusion", 501), ("fusion_c", 401), ("fusion_c", 301), ("fusion_c", 201),
                    ("fusion_base_c", 101), ("plain_c", 1)], traj


def test_order_rule_at_both_borders():
    """solver='dpmpp2m': a step is second order (c1 != 0) only when the step before was a solver step of the same mode AND the same guidedness.
    n = 20 on the leading grid, fusion from 751 on, interval (700, 250): 701 is the last unguided fusion step before the interval, 651 the first
    guided one, 251 the last guided one, 201 the first unguided one behind it"""
    tw, calls = _recorded_run(n=20, guidance_interval=GC.INTERVAL, solver="dpmpp2m")
    ts = tw.scheduler.timesteps
    assert ts[:6] == [951, 901, 851, 801, 751, 701]
    steps = {t: (k, ms) for k, _m, t, ms in calls if ms is not None}
    assert set(steps) == set(ts[1:])                                             # every timestep behind the first is a solver step
    order = {t: (2 if ms[2] != 0.0 else 1) for t, (_k, ms) in steps.items()}
    kinds = {t: k for t, (k, _ms) in steps.items()}
    assert kinds[901] == kinds[851] == kinds[801] == "plain_c" and (order[901], order[851], order[801]) == (1, 2, 2)     # first solver step; then same mode, all unguided
    assert kinds[751] == kinds[701] == "fusion_c" and (order[751], order[701]) == (1, 2)         # the mode changes; then second order again
    assert kinds[651] == "fusion" and order[651] == 1                                           # upper border: guidedness changes
    assert kinds[601] == "fusion" and order[601] == 2
    assert kinds[251] == "fusion" and order[251] == 2
    assert kinds[201] == "fusion_c" and order[201] == 1                                         # lower border
    assert kinds[151] == "fusion_c" and order[151] == 2
    assert order[1] == 1 and steps[1][1] == (0.0, 1.0, 0.0)                                      # the last step writes x0
    # without an interval the same run is second order across both places
    _, plain = _recorded_run(n=20, solver="dpmpp2m")
    o2 = {t: (2 if ms[2] != 0.0 else 1) for _k, _m, t, ms in plain if ms is not None}
    assert o2[651] == 2 and o2[201] == 2 and all(not k.endswith("_c") for k, *_ in plain)
    assert {t: v for t, v in o2.items() if t not in (651, 201)} == {t: v for t, v in order.items() if t not in (651, 201)}


# ------------------------------------------------------------------------------------------------ defaults
@pytest.mark.parametrize("kw", [{}, dict(solver="dpmpp2m", timestep_spacing="logsnr")], ids=["ddim", "dpmpp2m_logsnr"])
def test_full_interval_is_the_run_without_the_argument(kw):
    base_tw, base = _recorded_run(**kw)
    for interval in ((1000, 0), (901, 1), "901,1"):
        tw, calls = _recorded_run(guidance_interval=interval, **kw)
        assert calls == base and tw.unet_calls == base_tw.unet_calls and len(tw.unet_calls) == 13
    assert all(not k.endswith("_c") for k, *_ in base)
    assert base_tw._n_params == 8 and _recorded_run(guidance_interval=GC.INTERVAL)[0]._n_params == 8            # the upload size is unchanged


def test_plan_kinds_rows_and_weight_sets(monkeypatch):
    """_build_plan on the host (plans replaced by recorders): the unguided kinds drop exactly the unconditional row -- prompts te[2:2+K] on weight
    sets 1..K (fusion_c, routed like its twin) or set 0 (fusion_base_c), te[1] alone (plain_c) -- seed-major for co-batched seeds, fp8 passed
    through, and --streams 2 splits by its existing divisibility rule only"""
    from tweediemix_amd import sampler as S
    made = []

    class KV:
        def __init__(self, W, ehs, wsel):
            self.ehs, self.wsel = ehs, list(wsel)

    class Plan:
        def __init__(self, W, B, h, w, kv, pooled, tid, routed=False, row_sets=None, fp8=False):
            made.append(("plan", B, kv.ehs, kv.wsel, pooled, routed, row_sets, fp8))
            self.B = B

    class Group:
        def __init__(self, W, h, w, ehs, wsel, pooled, tid, routed, n, fp8=False):
            made.append(("group", ehs.shape[0], ehs, list(wsel), pooled, routed, n, fp8))
            self.B = ehs.shape[0]
    monkeypatch.setattr(S, "KVCache", KV)
    monkeypatch.setattr(S, "UNetPlan", Plan)
    monkeypatch.setattr(S, "PlanGroup", Group)
    K = 3
    te = (torch.arange(K + 2, dtype=torch.float32).reshape(-1, 1, 1).repeat(1, 77, 8), torch.arange(K + 2, dtype=torch.float32).reshape(-1, 1).repeat(1, 6))
    W = GC.NoWeights("cpu")
    W.kind = "lora"
    for seeds, streams in ((1, 1), (2, 1), (1, 2), (2, 2)):
        tw = S.Tweediemix(GC.make_cfg(S), W, te, te, None, concept_num=K, n_seeds=seeds, n_streams=streams, fp8=True, guidance_interval=GC.INTERVAL)
        for kind, rows, sets, routed in (("fusion_c", [2, 3, 4], [1, 2, 3], True), ("fusion_base_c", [2, 3, 4], [0, 0, 0], False),
                                         ("plain_c", [1], [0], False)):
            made.clear()
            p = tw.plan(kind)
            what, B, ehs, wsel, pooled, r, extra, fp8 = made[0]
            assert B == p.B == seeds * len(rows) and fp8 is True and r is routed, (kind, seeds, streams)
            assert ehs[:, 0, 0].tolist() == rows * seeds and pooled[:, 0].tolist() == rows * seeds and wsel == sets * seeds
            split = streams == 2 and B % 2 == 0 and B // 2 >= 2                   # 3 rows, 1 row and 2 x 1 rows run as one chain
            assert what == ("group" if split else "plan"), (kind, seeds, streams)
            if what == "plan":
                assert extra == (wsel if routed else None)
            assert tw.plan(kind) is p and len(made) == 1                          # built lazily, once
        assert set(tw.plans) == {"fusion_c", "fusion_base_c", "plain_c"}
    # strict_reference keeps the reference's batch == 4 test on the guided twin's batch: K = 2 routes neither
    te2 = (te[0][:4], te[1][:4])
    tw = S.Tweediemix(GC.make_cfg(S), W, te2, te2, None, concept_num=2, guidance_interval=GC.INTERVAL)
    made.clear()
    tw.plan("fusion_c")
    assert made[0][3] == [0, 0] and made[0][5] is False


# ------------------------------------------------------------------------------------------------ the entry's argument checks (no launch, no GPU)
def test_cond_entry_validates_like_its_siblings():
    """tmix_fused_tweedie_step_cond_dev answers a bad argument with check_dev_step's codes and wording under its own name, needs one eps row less
    than its siblings (there is no unconditional row), refuses RESAMPLE, and reads the window arguments only when it is handed keys"""
    import ctypes as C
    from tweediemix_amd import lib
    l = lib.load()
    f = C.c_void_p(0x1000)                      # never dereferenced: validation fails first
    ok = dict(x=f, eps=f, dt=lib.F32, masks=f, mss=0, out_x=f, out_x0=None, K=3, C=4, hw=64, mode=lib.STEP_FUSION, rows=3, seeds=2, prm=f)
    tail = dict(prev=None, keys=f, w=8, n_win=1, yx=None, ch=0, cw=0)

    def call(**kw):
        h = dict(ok, **{k: v for k, v in kw.items() if k in ok})
        t = dict(tail, **{k: v for k, v in kw.items() if k in tail})
        if t["yx"] is not None:
            t["yx"] = (C.c_int32 * len(t["yx"]))(*t["yx"])
        return l.tmix_fused_tweedie_step_cond_dev(*h.values(), *t.values(), None)
    err = l.tmix_last_error_string
    own = b"tweedie_step_cond_dev: "
    bad = [(dict(x=None), lib.EINVAL, b"null pointer"), (dict(eps=None), lib.EINVAL, b"null pointer"), (dict(out_x=None), lib.EINVAL, b"null pointer"),
           (dict(prm=None), lib.EINVAL, b"null pointer"), (dict(mode=-1), lib.EINVAL, b"bad mode -1 (FUSION or PLAIN)"),
           (dict(mode=lib.STEP_RESAMPLE), lib.EINVAL, b"bad mode 2 (FUSION or PLAIN)"), (dict(masks=None), lib.EINVAL, b"FUSION needs masks and K>=1"),
           (dict(K=0), lib.EINVAL, b"FUSION needs masks and K>=1"), (dict(C=0), lib.ESHAPE, b"channels=0 hw=64 seeds=2"),
           (dict(hw=0), lib.ESHAPE, b"channels=4 hw=0 seeds=2"), (dict(seeds=0), lib.ESHAPE, b"channels=4 hw=64 seeds=0"),
           (dict(seeds=65536), lib.ESHAPE, b"channels=4 hw=64 seeds=65536"), (dict(rows=2), lib.ESHAPE, b"mode 0 needs 3 eps rows per seed, got 2"),
           (dict(mode=lib.STEP_PLAIN, rows=0, masks=None), lib.ESHAPE, b"mode 1 needs 1 eps rows per seed, got 0"),
           (dict(n_win=0), lib.EINVAL, b"n_win=0"), (dict(n_win=2), lib.EINVAL, b"n_win=2"), (dict(n_win=9, yx=[0] * 18), lib.EINVAL, b"n_win=9"),
           (dict(w=5), lib.ESHAPE, b"hw=64 is not a multiple of the row width w=5"),
           (dict(n_win=2, yx=[0, 0, 0, 3], ch=8, cw=10), lib.ESHAPE, b"window 1 at (0, 3) of 8 x 8 reaches outside the 8 x 10 canvas"),
           (dict(n_win=2, yx=[0, 0, 0, 2], ch=8, cw=10, seeds=3), lib.ESHAPE, b"seeds=3 is not a multiple of n_win=2"),
           (dict(dt=7), lib.EINVAL, b"bad eps dtype 7")]
    for kw, code, text in bad:
        for prev in (None, f):                  # the history buffer is optional: the answers do not depend on it
            assert call(prev=prev, **kw) == code, (kw, err())
            assert err().startswith(own + text), (kw, err())
    # without keys the window arguments are not looked at: the call gets past them to the dtype check
    for kw in (dict(n_win=0), dict(w=5), dict(n_win=2, yx=[0, 0, 0, 3], ch=8, cw=10)):
        assert call(keys=None, dt=7, **kw) == lib.EINVAL and err().startswith(own + b"bad eps dtype 7"), (kw, err())
