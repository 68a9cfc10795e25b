"""CPU: stochastic sampling of the VIDEO sampler -- the coefficients on the video table's edge cases, the numpy restatement of
tmix_vpred_step_noise / tmix_vpred_step_noise_dev against its four parents, the stream id, the ABI's refusals, the refusals of sample_loop,
VideoSampler and run_video.py before the GPU, and the Gaussian model of the video loop (tests/video_noise_cases.py)."""
import importlib.util
import os
import types

import numpy as np
import pytest
import torch

import video_noise_cases as VN
from video_solver_cases import standin_schedule, standin_table

NF = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOWPS = [None, np.float16, "bf16"]


# ------------------------------------------------------------------------------------------------ coefficients
@pytest.mark.parametrize("spacing", ["leading", "logsnr"])
@pytest.mark.parametrize("n", [10, 20, 50])
def test_eta_zero_is_todays_coefficients_and_eta_one_coincides(n, spacing):
    """on the stand-in table, every step of the grid, the step to final_alpha_cumprod included: eta = 0 gives video_multistep_coeffs' and
    ops.step_coeffs' values bit for bit and cz == 0.0; at eta = 1 DDIM in the form cx x + c0 x0 + cz z (eps = (x - sa x0) / s1) is the solver's
    first-order step to fp64 rounding (the tolerance of tests/test_noise_cpu.py); SolverPhase hands out the same values with its own bookkeeping"""
    from tweediemix_amd import ops, solver as SV, video as V
    sch = standin_schedule(n, spacing)
    ts = [int(t) for t in sch.timesteps]
    plain, zero, one = V.SolverPhase(sch), V.SolverPhase(sch), V.SolverPhase(sch)
    for i, t in enumerate(ts):
        a, an = sch.alpha(t), sch.next_alpha(t)
        ap = sch.alpha(ts[i - 1]) if i else None
        assert SV.ddim_eta_coeffs(a, an, 0.0) == ops.step_coeffs(a, an) + (0.0,)
        for second in ((False, True) if i else (False,)):
            want = SV.video_multistep_coeffs(t, ap, a, an, second)
            got = SV.video_multistep_eta_coeffs(t, ap, a, an, second, 0.0)
            assert got == want + (0.0,) and got[3] == 0.0
            assert SV.video_multistep_eta_coeffs(t, ap, a, an, second, 0.6) == SV.multistep_eta_coeffs(ap, a, an, second, 0.6)
        sa, s1, san, s1d, cz = SV.ddim_eta_coeffs64(a, an, 1.0)
        cx, c0, c1, cz2 = SV.multistep_eta_coeffs64(ap, a, an, False, 1.0)
        assert c1 == 0.0 and cz > 0.0
        assert abs(s1d / s1 - cx) <= 1e-12 * cx and abs(san - s1d * sa / s1 - c0) <= 1e-12 * san and abs(cz - cz2) <= 1e-12 * cz
        three = plain.coeffs(t)
        assert len(three) == 3 and zero.coeffs(t, 0.0) == three + (0.0,)
        four = one.coeffs(t, 1.0)
        assert four == SV.multistep_eta_coeffs(ap, a, an, i > 0, 1.0) and four[3] > 0.0 and (four[2] == 0.0) == (i == 0)


def test_coefficients_on_the_tables_edges():
    """a_next >= 1 (set_alpha_to_one behind the last entry) lands on the data: (0, 1, 0) and cz == 0 at every eta, DDIM's sigma is 0 there too;
    a == 0 has no log-SNR and is refused as video_multistep_coeffs refuses it"""
    from tweediemix_amd import solver as SV, video as V
    for eta in (0.0, 0.5, 1.0):
        assert SV.video_multistep_eta_coeffs(1, 0.9, 0.99, 1.0, True, eta) == (0.0, 1.0, 0.0, 0.0)
        assert SV.video_multistep_eta_coeffs(1, None, 0.99, NF(1.0), False, eta) == (0.0, 1.0, 0.0, 0.0)
        assert SV.ddim_eta_coeffs(0.99, 1.0, eta)[3:] == (0.0, 0.0)
        with pytest.raises(ValueError, match=r"alpha\(999\)"):
            SV.video_multistep_eta_coeffs(999, None, 0.0, 0.1, False, eta)
    acp, kw = standin_table()
    one = V.VideoSchedule(acp, 10, steps_offset=1, set_alpha_to_one=True, spacing="logsnr")
    ph = V.SolverPhase(one)
    cf = [ph.coeffs(int(t), 1.0) for t in one.timesteps]
    assert cf[-1] == (0.0, 1.0, 0.0, 0.0) and all(c[3] > 0.0 for c in cf[:-1])
    with pytest.raises(ValueError, match=r"alpha\(999\)"):
        V.SolverPhase(V.VideoSchedule(acp, 50, **kw)).coeffs(999, 1.0)


# ------------------------------------------------------------------------------------------------ restatement
def _case(B=2, n=70, seed=3, lowp=None):
    rng = np.random.RandomState(seed)
    q = (lambda a: a.astype(np.float16).astype(NF)) if lowp is np.float16 else (lambda a: torch.from_numpy(a).bfloat16().float().numpy()) if lowp == "bf16" \
        else (lambda a: a)
    x, v, prev = q(rng.randn(B, n).astype(NF)), q(rng.randn(2 * B, n).astype(NF)), rng.randn(B, n).astype(NF)
    return x, v, prev, (0.4 + 0.6 * rng.rand(B)).astype(NF)


G_, SA, S1, A, B_, C_ = 9.0, float(np.sqrt(NF(0.2345))), float(np.sqrt(NF(1) - NF(0.2345))), 0.8125, 0.4021, -0.0804


@pytest.mark.parametrize("lowp", LOWPS, ids=["f32", "f16", "bf16"])
def test_restatement_at_cz_zero_is_the_four_parents(lowp):
    """both argument forms (the dense entry's seven coefficients, the _dev entry's twelve parameters) against tmix_vpred_step / _ms (the restatements
    of the solver tests), _rs / _ms_rs (guidance.vpred_rescaled_*), by equality, output and x0"""
    from oracle import tweedie_oracle as TO
    from tweediemix_amd import guidance as GD, noise as NZ, solver as SV
    x, v, prev, fac = _case(lowp=lowp)
    keys = VN.KEYS[:2]
    dd7, ms7 = (G_, SA, S1, A, B_, 0.0, 0.0), (G_, SA, S1, A, B_, C_, 0.0)
    dd12, ms12 = [501.0, SA, S1, A, B_, G_, 0.0, 0.0, 0.0, 7.0, 0.0, 0.0], [501.0, SA, S1, A, B_, C_, G_, 0.0, 0.0, 7.0, 0.0, 0.0]
    for f in (None, fac):
        ff = np.ones(2, NF) if f is None else f
        want = GD.vpred_rescaled_step_reference(x, v, ff, G_, SA, S1, A, B_, lowp)
        for got in (NZ.vpred_step_reference(x, v, None, dd7, keys, 7, f, lowp), NZ.vpred_step_reference(x, v, None, dd12, keys, None, f, lowp)):
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        want = GD.vpred_rescaled_multistep_reference(x, v, prev, ff, G_, SA, S1, A, B_, C_, lowp)
        for got in (NZ.vpred_step_reference(x, v, prev, ms7, keys, 7, f, lowp), NZ.vpred_step_reference(x, v, prev, ms12, keys, None, f, lowp)):
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    # ... and the unscaled parents: the multistep restatement of the solver tests, and in fp32 the oracle's DDIM formula (sa', s1' from an alpha)
    want = SV.vpred_multistep_reference(x, v, prev, G_, SA, S1, A, B_, C_, lowp)
    got = NZ.vpred_step_reference(x, v, prev, ms7, keys, 7, None, lowp)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    if lowp is None:
        at, an = NF(0.2345), NF(0.2871)
        want = TO.video_vpred_step(x, v, G_, at, an)
        got = NZ.vpred_step_reference(x, v, None, (G_, SA, S1, float(np.sqrt(an)), float(np.sqrt(NF(1) - an)), 0.0, 0.0), keys, 7)
        assert np.array_equal(got[0], np.asarray(want, NF))


@pytest.mark.parametrize("lowp", LOWPS, ids=["f32", "f16", "bf16"])
def test_restatement_adds_exactly_the_rounded_product_on_a_zero_input(lowp):
    """x = v = 0, history 0: moved is 0, so the output is rnd(cz z) of the video's own key -- the fp16 product rounded to fp16, the bf16 store rounded
    once -- and a non-zero input gets one product and one sum behind the parent's move"""
    from tweediemix_amd import noise as NZ, solver as SV
    B, n = 3, 70
    z0 = np.zeros((B, n), NF)
    z = VN.video_noise(n, VN.KEYS, VN.STEP)
    prod = (NF(VN.CZ) * z).astype(NF)
    rnd = {None: prod, np.float16: prod.astype(np.float16).astype(NF), "bf16": SV._bf16_round(prod)}[lowp]
    for prev, co in ((None, (G_, SA, S1, A, B_, 0.0, VN.CZ)), (z0, (G_, SA, S1, A, B_, C_, VN.CZ))):
        out, x0 = NZ.vpred_step_reference(z0, np.zeros((2 * B, n), NF), prev, co, VN.KEYS, VN.STEP, None, lowp)
        assert np.array_equal(out, rnd) and not x0.any()
    assert not np.array_equal(z[0], z[1]) and np.abs(z).max() < 5.8
    x, v, prev, fac = _case(B=3, lowp=lowp)
    lp = None if lowp == "bf16" else lowp
    base = NZ.vpred_step_reference(x, v, prev, (G_, SA, S1, A, B_, C_, 0.0), VN.KEYS, VN.STEP, fac, lp)
    got = NZ.vpred_step_reference(x, v, prev, (G_, SA, S1, A, B_, C_, VN.CZ), VN.KEYS, VN.STEP, fac, lowp)
    want = SV._h((base[0] + SV._h(prod, lp)).astype(NF), lp)
    assert np.array_equal(got[0], SV._bf16_round(want) if lowp == "bf16" else want) and np.array_equal(got[1], base[1])
    twelve = [501.0, SA, S1, A, B_, C_, G_, 0.0, VN.CZ, float(VN.STEP), 0.0, 0.0]
    assert np.array_equal(NZ.vpred_step_reference(x, v, prev, twelve, VN.KEYS, None, fac, lowp)[0], got[0])
    with pytest.raises(ValueError, match="keys"):
        NZ.vpred_step_reference(x, v, prev, twelve, VN.KEYS[:2])
    with pytest.raises(ValueError, match="12 device parameters"):
        NZ.vpred_step_reference(x, v, prev, twelve[:8], VN.KEYS)


def test_the_video_stream_draws_other_noise_than_the_image_stream():
    from tweediemix_amd import noise as NZ
    assert (NZ.STREAM_IMAGE_STEP, NZ.STREAM_VIDEO_STEP) == (0, 1)
    idx = np.arange(4096, dtype=np.uint64)
    a, b = NZ.normal(idx, 182, 0, 7, NZ.STREAM_IMAGE_STEP), NZ.normal(idx, 182, 0, 7, NZ.STREAM_VIDEO_STEP)
    assert np.array_equal(a, NZ.normal(idx, 182, 0, 7)) and not (a == b).any()
    assert abs(float(np.corrcoef(a, b)[0, 1])) < 5 / np.sqrt(4096)            # five standard errors of a correlation of independent draws
    assert np.array_equal(VN.video_noise(4096, [(182, 0)], 7)[0], b)
    src = open(os.path.join(ROOT, "tweediemix_amd", "csrc", "noise.h")).read()
    assert "STREAM_VIDEO_STEP" in src


# ------------------------------------------------------------------------------------------------ ABI
def test_entries_are_declared_and_validate_before_any_launch():
    from tweediemix_amd import lib
    l = lib.load()
    src = open(os.path.join(ROOT, "include", "tmix.h")).read()
    assert "int tmix_vpred_step_noise(" in src and "int tmix_vpred_step_noise_dev(" in src
    err = l.tmix_last_error_string
    f = 0x1000                                                  # never dereferenced: validation fails first
    ok = dict(x=f, v=f, out=f, prev=None, dt=lib.F32, S=2, n=64, fac=None, keys=f)

    def dense(**kw):
        a = dict(ok, **kw)
        return l.tmix_vpred_step_noise(a["x"], a["v"], a["out"], a["prev"], a["dt"], a["S"], a["n"], 9.0, 0.6, 0.8, 0.7, 0.5, 0.0, 0.25, a["fac"], a["keys"], 7, None)
    okd = dict(x=f, vu=f, su=4 * 2 * 8, vc=f, sc=4 * 2 * 8, prm=f, S=2, C=4, F=2, hw=8, prev=None, fac=None, keys=f)

    def rows(**kw):
        a = dict(okd, **kw)
        return l.tmix_vpred_step_noise_dev(a["x"], a["vu"], a["su"], a["vc"], a["sc"], a["prm"], a["S"], a["C"], a["F"], a["hw"], a["prev"], a["fac"], a["keys"], None)
    for forms in (dict(), dict(prev=f), dict(fac=f), dict(prev=f, fac=f)):
        for k in ("x", "v", "out"):
            assert dense(**forms, **{k: None}) == lib.EINVAL and b"null" in err(), k
        for k in ("x", "vu", "vc", "prm"):
            assert rows(**forms, **{k: None}) == lib.EINVAL and b"null" in err(), k
        for call in (dense, rows):
            assert call(**forms, keys=None) == lib.EINVAL and b"null keys" in err()
            assert call(**forms, S=0) == lib.ESHAPE and b"videos=0" in err()
        assert dense(**forms, dt=7) == lib.EINVAL and b"dtype" in err()
        assert dense(**forms, n=0) == lib.ESHAPE
        for bad in (dict(C=0), dict(F=0), dict(hw=0)):
            assert rows(**forms, **bad) == lib.ESHAPE, bad
        assert rows(**forms, su=63) == lib.ESHAPE and b"clip stride" in err()
        assert rows(**forms, sc=63) == lib.ESHAPE


def test_ops_wrappers_refuse_cpu_tensors():
    from tweediemix_amd import lib, ops
    x, v, keys = torch.zeros(1, 4, 2, 2, 2), torch.zeros(2, 4, 2, 2, 2), torch.zeros(1, 2, dtype=torch.int32)
    with pytest.raises(lib.TmixError):
        ops.vpred_step_noise(x, v, 9.0, 0.3, (0.6, 0.7), 0.25, keys, 3)
    with pytest.raises(lib.TmixError):
        ops.vpred_step_noise(x, v, 9.0, 0.3, (0.8, 0.4, -0.1), 0.25, keys, 3, x0_prev=torch.zeros_like(x))
    with pytest.raises(lib.TmixError):
        ops.vpred_step_noise_dev(x, torch.zeros(2, 4, 2, 2), torch.zeros(2, 4, 2, 2), torch.zeros(12), keys)
    p = ops.video_step_params_noise(501, 9.0, NF(0.2345), (0.8, 0.4, -0.1), 0.25, 3)
    assert p.dtype == torch.float32 and p.tolist() == [501.0, SA, S1, float(NF(0.8)), float(NF(0.4)), float(NF(-0.1)), 9.0, 0.0, 0.25, 3.0, 0.0, 0.0]
    slot = torch.full((12,), -1.0)
    assert ops.video_step_params_noise(501, 9.0, NF(0.2345), (0.6, 0.7), 0.25, 3, out=slot) is slot
    assert slot.tolist() == [501.0, SA, S1, float(NF(0.6)), float(NF(0.7)), 9.0, 0.0, 0.0, 0.25, 3.0, 0.0, 0.0]
    assert slot[:8].tolist() == ops.video_step_params(501, 9.0, NF(0.2345), NF(0.2871)).tolist()[:3] + slot[3:8].tolist()      # the parent's head
    with pytest.raises(AssertionError):
        ops.video_step_params_noise(501, 9.0, NF(0.2345), (0.6, 0.7), 0.25, 2 ** 24)


# ------------------------------------------------------------------------------------------------ refusals before the GPU
def _no_gpu(monkeypatch):
    def no_gpu(*a, **k):
        raise AssertionError("the GPU was touched before the refusal")
    for name in ("init", "_lazy_init", "set_device", "current_stream"):
        monkeypatch.setattr(torch.cuda, name, no_gpu)


def test_sampler_and_loop_refusals_come_before_the_gpu(monkeypatch):
    from tweediemix_amd import video as V
    _no_gpu(monkeypatch)
    sch = standin_schedule(10, "logsnr")
    plan = types.SimpleNamespace(videos=2)                      # nothing else of the plan is read before the refusal
    x = torch.zeros(2, 4, 2, 4, 4)
    net = lambda xin, t: (_ for _ in ()).throw(AssertionError("the network ran"))
    for solver in V.SOLVERS:
        for bad in (-0.1, 1.5, float("nan"), "much"):
            with pytest.raises(ValueError, match="eta"):
                V.VideoSampler(plan, sch, 9.0, solver=solver, eta=bad, noise_seeds=[1, 2])
            with pytest.raises(ValueError, match="eta"):
                V.sample_loop(net, x, sch, 9.0, solver=solver, eta=bad, noise_seeds=[1, 2])
        with pytest.raises(ValueError, match="noise_seeds"):
            V.VideoSampler(plan, sch, 9.0, solver=solver, eta=0.5)
        with pytest.raises(ValueError, match="noise_seeds"):
            V.sample_loop(net, x, sch, 9.0, solver=solver, eta=0.5)
        for seeds in ([1], [1, 2, 3], []):
            with pytest.raises(ValueError, match=rf"{len(seeds)} values for 2 videos"):
                V.VideoSampler(plan, sch, 9.0, solver=solver, eta=0.5, noise_seeds=seeds)
            with pytest.raises(ValueError, match=rf"{len(seeds)} values for 2 videos"):
                V.sample_loop(net, x, sch, 9.0, solver=solver, eta=0.5, noise_seeds=seeds)
    # a timestep off the grid has no schedule index: refused by the host bookkeeping (a 'leading' grid would otherwise step from it)
    with pytest.raises(ValueError, match="not one of the schedule's timesteps"):
        V._noise_step(standin_schedule(10), 650, 0.5, None)
    move, cz, i = V._noise_step(standin_schedule(10), 601, 0.5, None)
    assert i == 3 and len(move) == 2 and cz > 0.0
    move, cz, i = V._noise_step(sch, int(sch.timesteps[0]), 1.0, V.SolverPhase(sch))
    assert i == 0 and len(move) == 3 and move[2] == 0.0 and cz > 0.0        # the first step is a first-order SOLVER step and takes noise


@pytest.fixture(scope="module")
def rv():
    spec = importlib.util.spec_from_file_location("rv_noise_cpu", os.path.join(ROOT, "run_video.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_cli_eta_refusals_come_before_the_gpu(rv, monkeypatch):
    opt = rv.build_parser().parse_args([])
    assert opt.eta == 0.0 and rv.checked_eta(opt) == 0.0
    opt = rv.build_parser().parse_args(["--eta", "0.5", "--solver", "dpmpp2m"])
    assert rv.checked_eta(opt) == 0.5
    assert "--eta" in rv.__doc__ and "--eta" in rv.build_parser().format_help()
    _no_gpu(monkeypatch)
    started = []
    from tweediemix_amd import launch as LA
    monkeypatch.setattr(LA, "self_launch", lambda n: started.append(n))
    for bad in ("-0.1", "1.5", "nan"):
        for more in ([], ["--gpus", "2"], ["--solver", "dpmpp2m", "--timestep_spacing", "logsnr", "--num_seeds", "2"]):
            with pytest.raises(SystemExit, match=r"--eta"):
                rv.main(["--synthetic", "--tiny", "--eta=" + bad] + more)
    assert started == []                                        # ... and before any rank starts
    with pytest.raises(SystemExit):
        rv.build_parser().parse_args(["--eta", "much"])
    # a video's key is the seed of its x_T; the padding of a ragged last batch takes the key of the batch's last real video
    assert rv.batch_noise_seeds([7, 8, 9], 3) == [7, 8, 9]
    assert rv.batch_noise_seeds([7, 8, 7, 8], 2) == [7, 8, 8, 8] and rv.batch_noise_seeds([9, 9], 1) == [9, 9]


# ------------------------------------------------------------------------------------------------ Gaussian model
def test_variance_on_the_gaussian_model_of_the_video_loop():
    """data N(0, c^2), eta = 1, the closed-form covariance recursion of tests/video_noise_cases.py on the stand-in table: relative error of the
    variance of the final state (at final_alpha_cumprod) against a_f c^2 + 1 - a_f.  The table, as this test prints it (c = 0.5 / 1 / 2):
    dpmpp2m logsnr n = 10, 20, 40: 9.56e-2 4.29e-2 1.39e-2 / 9.98e-2 4.36e-2 1.37e-2 / 8.11e-2 4.33e-2 1.36e-2  (the result is too wide);
    ddim leading   n = 10, 20, 40: 3.96e-1 2.52e-1 1.49e-1 / 3.19e-1 1.88e-1 1.04e-1 / 3.22e-1 1.83e-1 9.83e-2  (too narrow).
    Asserted is what the table shows: every error shrinks with n, the solver is below DDIM at every n, and the solver at n = 20 is below DDIM at
    n = 40.  The recursion is deterministic: the pinned values hold to the 3 digits printed."""
    table = {"dpmpp2m": {0.5: (9.56e-2, 4.29e-2, 1.39e-2), 1.0: (9.98e-2, 4.36e-2, 1.37e-2), 2.0: (8.11e-2, 4.33e-2, 1.36e-2)},
             "ddim": {0.5: (3.96e-1, 2.52e-1, 1.49e-1), 1.0: (3.19e-1, 1.88e-1, 1.04e-1), 2.0: (3.22e-1, 1.83e-1, 9.83e-2)}}
    for c in VN.CS:
        ms = {n: VN.variance_error(c, n, "logsnr", "dpmpp2m") for n in VN.NS}
        dd = {n: VN.variance_error(c, n, "leading", "ddim") for n in VN.NS}
        print(f"c = {c}: dpmpp2m logsnr " + " ".join(f"{ms[n]:.2e}" for n in VN.NS) + "   ddim leading " + " ".join(f"{dd[n]:.2e}" for n in VN.NS))
        assert ms[10] > ms[20] > ms[40] and dd[10] > dd[20] > dd[40], c
        assert all(ms[n] < dd[n] for n in VN.NS) and ms[20] < dd[40], c
        for got, want in ((ms, table["dpmpp2m"][c]), (dd, table["ddim"][c])):
            assert all(abs(got[n] - w) <= 0.006 * w for n, w in zip(VN.NS, want)), (c, got, want)      # half a unit of the third digit
    # eta = 0 in the same recursion is the deterministic loop: no noise enters, and the variance is another one
    v0, sch = VN.predicted_variance(1.0, 20, "logsnr", "dpmpp2m", 0.0)
    v1, _ = VN.predicted_variance(1.0, 20, "logsnr", "dpmpp2m", 1.0)
    assert v0 > 0 and v0 != v1 and 0.99 < float(sch.final_alpha_cumprod) < 1.0
